// partial_valu.inc — part of kvq_attn.hip (one translation unit, included in this order): decode_attn_partial_k: the VALU split kernel (any head_dim, <= 8 query heads per kv head)
// Workgroup timeline (one round trip to HBM on the critical path when TS == TL * kAttnUnroll):
// issue the first K tile, the first V tile, the scales and the query at once; scores while V is
// still in flight; softmax in LDS; weighted V sum; token lanes -> one row per wave -> workspace.
// The body of decode_attn_partial_k (WIN = false) and of decode_attn_partial_window_k (WIN = true: a device-side count under
// a sliding window, its split rows start lo = window_lo rows into the store). Only the WIN instantiation evaluates the window.
// PAD (decode_attn_partial_padded_k: a left-padded batch, host or device count): lo = padded_lo of the workgroup's batch row,
// the larger of the window's bound and kv_start[b]; a split past the row's live count exits before it requests anything.
// CAP (decode_attn_partial_mod_k, a soft-capped kvq_*_ex call; built on PAD, the most general form): every scaled score becomes
// c tanh(s / c) before the split's softmax, and a NULL kv_start reads as 0.
template <int KBITS, int VBITS, int NQ, bool WIN, bool PAD = false, bool CAP = false>
__device__ __forceinline__ void decode_attn_partial_body(const AttnArgs a, const AttnMod mod = AttnMod{}) {
  __shared__ float s_p[NQ][kAttnMaxTS];  // raw scores, then p[t] * sv[t]
  __shared__ float s_ks[kAttnMaxTS];     // sk[t] * sm_scale
  __shared__ float s_vs[kAttnMaxTS];     // sv[t]
  __shared__ float s_acc[kAttnBlock / kWave][NQ][256];
  __shared__ float s_w[NQ];              // sum_t p[t] * sv[t]  (bias fold)
  const uint32_t tid = threadIdx.x;
  const uint32_t split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const uint32_t t0 = split * a.TS;
  uint32_t lo = 0u;  // WIN: the split's tokens start lo rows into the store
  uint32_t T;
  if constexpr (PAD) {
    T = live_tokens(a);
    int32_t start;
    if constexpr (CAP) start = a.kv_start ? kv_start_of(a, b) : 0;
    else start = kv_start_of(a, b);
    lo = padded_lo(a, T, start, a.kn != nullptr);
    T -= lo;
  } else if constexpr (WIN) T = live_window(a, lo);
  else T = live_tokens(a);
  if (t0 >= T) return;  // device-side T (graph replay): this split holds nothing yet
  const uint32_t nt = T - t0 < a.TS ? T - t0 : a.TS;
  const uint32_t r0 = t0 + lo;  // first stored row of the split
  const uint32_t lpt = 1u << a.lpt_shift;
  const uint32_t ld = tid & (lpt - 1u);    // which 16-element slice of D
  const uint32_t tl = tid >> a.lpt_shift;  // token lane
  const uint32_t TL = kAttnBlock >> a.lpt_shift;
  const uint32_t step = TL * kAttnUnroll;  // tokens per loop iteration

  const uint8_t* kb = a.k + (int64_t)b * a.k_sb + (int64_t)hk * a.k_sh + (int64_t)r0 * a.k_st +
                      (int64_t)ld * Raw16<KBITS>::kBytes;
  const uint8_t* vb = a.v + (int64_t)b * a.v_sb + (int64_t)hk * a.v_sh + (int64_t)r0 * a.v_st +
                      (int64_t)ld * Raw16<VBITS>::kBytes;
  // Every request of the prologue goes out before anything waits (one round trip): first K tile,
  // first V tile, query, scales. Rows past the split's end are CLAMPED to its last row instead of
  // skipped (no branches between the loads); their scores are never stored and their P never read.
  Raw16<KBITS> kraw[kAttnUnroll];
  Raw16<VBITS> vraw[kAttnUnroll];
#pragma unroll
  for (int u = 0; u < kAttnUnroll; ++u) {
    const uint32_t i = u * TL + tl;
    kraw[u].load(kb + (int64_t)(i < nt ? i : nt - 1u) * a.k_st);
  }
#pragma unroll
  for (int u = 0; u < kAttnUnroll; ++u) {
    const uint32_t i = u * TL + tl;
    vraw[u].load(vb + (int64_t)(i < nt ? i : nt - 1u) * a.v_st);
  }
  u32x4 qraw[NQ][2];
#pragma unroll
  for (int h = 0; h < NQ; ++h) {
    const uint32_t hh = (uint32_t)h < a.nq ? (uint32_t)h : 0u;  // padded heads read head 0, zeroed below
    const char* qp = reinterpret_cast<const char*>(a.q) +
                     ((int64_t)b * a.q_sb + (int64_t)(hk * a.nq + hh) * a.q_sh + (int64_t)ld * 16) * 2;
    qraw[h][0] = *reinterpret_cast<const u32x4*>(qp);
    qraw[h][1] = *(reinterpret_cast<const u32x4*>(qp) + 1);
  }
  {
    float ksv[kAttnMaxTS / kAttnBlock], vsv[kAttnMaxTS / kAttnBlock];
#pragma unroll
    for (int r = 0; r < kAttnMaxTS / kAttnBlock; ++r) {
      const uint32_t i = r * kAttnBlock + tid;
      const uint32_t ic = i < nt ? i : nt - 1u;
      ksv[r] = a.k_scale[r0 + ic];
      vsv[r] = a.v_scale[r0 + ic];
    }
#pragma unroll
    for (int r = 0; r < kAttnMaxTS / kAttnBlock; ++r) {
      const uint32_t i = r * kAttnBlock + tid;
      if (i < nt) {
        s_ks[i] = ksv[r] * a.sm_scale;
        s_vs[i] = vsv[r];
      }
    }
  }

  // ---- phase A: raw scores q . k_int ------------------------------------------------------
  {
    f16x2 qv[NQ][8];
#pragma unroll
    for (int h = 0; h < NQ; ++h) {
      if ((uint32_t)h < a.nq) {
        convert_q16<KBITS == 4>(qraw[h][0], qraw[h][1], a.dtype, qv[h]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) qv[h][j] = f16x2{(f16)0.0f, (f16)0.0f};
      }
    }
    for (uint32_t base = 0; base < nt; base += step) {  // uniform trip count
      const bool more = base + step < nt;
      Raw16<KBITS> nxt[kAttnUnroll];
      if (more) {  // next tile in flight while this one is reduced
#pragma unroll
        for (int u = 0; u < kAttnUnroll; ++u) {
          const uint32_t i = base + step + u * TL + tl;
          nxt[u].load(kb + (int64_t)(i < nt ? i : nt - 1u) * a.k_st);
        }
      }
#pragma unroll
      for (int u = 0; u < kAttnUnroll; ++u) {
        const uint32_t i = base + u * TL + tl;
        f16x2 kp[8];
        kraw[u].to_h2(kp);
#pragma unroll
        for (int h = 0; h < NQ; ++h) {
          float s = 0.0f;
#pragma unroll
          for (int j = 0; j < 8; ++j) s = __builtin_amdgcn_fdot2(kp[j], qv[h][j], s, false);
          s = group_fadd(s, a.lpt_shift);
          if (ld == 0u && i < nt) s_p[h][i] = s;
        }
      }
      if (more) {
#pragma unroll
        for (int u = 0; u < kAttnUnroll; ++u) kraw[u] = nxt[u];
      }
    }
  }
  __syncthreads();

  // ---- phase B: per-head softmax over this split (one wave per head, round robin) -----------
  {
    const uint32_t wave = tid >> 6, lane = tid & 63u;
    for (uint32_t h = wave; h < a.nq; h += kAttnBlock / kWave) {
      float m = -INFINITY;
      for (uint32_t i = lane; i < nt; i += kWave) {
        float sc = s_p[h][i] * s_ks[i];
        if constexpr (CAP) sc = softcap_score(sc, mod);
        s_p[h][i] = sc;
        m = fmaxf(m, sc);
      }
      m = wave_fmax(m);
      float l = 0.0f, wsum = 0.0f;
      for (uint32_t i = lane; i < nt; i += kWave) {
        const float p = __expf(s_p[h][i] - m);
        const float pv = p * s_vs[i];
        l += p;
        wsum += pv;
        s_p[h][i] = pv;
      }
      l = wave_fsum(l);
      wsum = wave_fsum(wsum);
      if (lane == 0u) {
        s_w[h] = wsum;
        float* o = a.ws + (((int64_t)b * a.Hq + hk * a.nq + h) * a.nsplit + split) * 2;
        o[0] = m;
        o[1] = l;
      }
    }
  }
  __syncthreads();

  // ---- phase C: acc[h][d] = sum_t (p sv)[t] * (v_int[t,d] + bias) ----------------------------
  float acc[NQ][16];
#pragma unroll
  for (int h = 0; h < NQ; ++h)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[h][j] = 0.0f;
  for (uint32_t base = 0; base < nt; base += step) {
    const bool more = base + step < nt;
    Raw16<VBITS> nxt[kAttnUnroll];
    if (more) {
#pragma unroll
      for (int u = 0; u < kAttnUnroll; ++u) {
        const uint32_t i = base + step + u * TL + tl;
        nxt[u].load(vb + (int64_t)(i < nt ? i : nt - 1u) * a.v_st);
      }
    }
#pragma unroll
    for (int u = 0; u < kAttnUnroll; ++u) {
      const uint32_t i = base + u * TL + tl;
      if (i < nt) {
        float uf[16];
        vraw[u].to_f32_biased(uf);
#pragma unroll
        for (int h = 0; h < NQ; ++h) {
          const float p = s_p[h][i];
#pragma unroll
          for (int j = 0; j < 16; ++j) acc[h][j] = fmaf(uf[j], p, acc[h][j]);
        }
      }
    }
    if (more) {
#pragma unroll
      for (int u = 0; u < kAttnUnroll; ++u) vraw[u] = nxt[u];
    }
  }
  // token lanes of one wave -> every lane holds the wave's sum, then the 4 waves through LDS.
  // Inside a 16-lane row: DPP rotations (one VALU op each); across rows: two lane exchanges per
  // value, issued back to back (the uniform branches stay OUTSIDE the value loops so that they pipeline).
#define KVQ_ROW_ROR(N)                                                                                     \
  _Pragma("unroll") for (int h = 0; h < NQ; ++h) _Pragma("unroll") for (int j = 0; j < 16; ++j)           \
      acc[h][j] += __uint_as_float(dpp_u32_attn<0x120 + N>(__float_as_uint(acc[h][j])));
  if (lpt <= 8u) { KVQ_ROW_ROR(8) }
  if (lpt <= 4u) { KVQ_ROW_ROR(4) }
  if (lpt <= 2u) { KVQ_ROW_ROR(2) }
  if (lpt <= 1u) { KVQ_ROW_ROR(1) }
#undef KVQ_ROW_ROR
#pragma unroll
  for (int h = 0; h < NQ; ++h) {
    float t[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) t[j] = __shfl_xor(acc[h][j], 16);
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[h][j] += t[j];
#pragma unroll
    for (int j = 0; j < 16; ++j) t[j] = __shfl_xor(acc[h][j], 32);
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[h][j] += t[j];
  }
  {
    const uint32_t wave = tid >> 6, lane = tid & 63u;
    if (lane < lpt) {
#pragma unroll
      for (int h = 0; h < NQ; ++h)
#pragma unroll
        for (int j = 0; j < 16; ++j) s_acc[wave][h][lane * 16 + j] = acc[h][j];
    }
  }
  __syncthreads();
  for (uint32_t idx = tid; idx < a.nq * a.D; idx += kAttnBlock) {
    const uint32_t h = idx / a.D, d = idx - h * a.D;
    const float v = s_acc[0][h][d] + s_acc[1][h][d] + s_acc[2][h][d] + s_acc[3][h][d] -
                    Raw16<VBITS>::kBias * s_w[h];
    a.ws[a.acc_off + (((int64_t)b * a.Hq + hk * a.nq + h) * a.nsplit + split) * a.D + d] = v;
  }
}

template <int KBITS, int VBITS, int NQ>
__global__ __launch_bounds__(kAttnBlock) void decode_attn_partial_k(const AttnArgs a) {
  decode_attn_partial_body<KBITS, VBITS, NQ, false>(a);
}
template <int KBITS, int VBITS, int NQ>
__global__ __launch_bounds__(kAttnBlock) void decode_attn_partial_window_k(const AttnArgs a) {
  decode_attn_partial_body<KBITS, VBITS, NQ, true>(a);
}
template <int KBITS, int VBITS, int NQ>
__global__ __launch_bounds__(kAttnBlock) void decode_attn_partial_padded_k(const AttnArgs a) {
  decode_attn_partial_body<KBITS, VBITS, NQ, true, true>(a);
}
template <int KBITS, int VBITS, int NQ>
__global__ __launch_bounds__(kAttnBlock) void decode_attn_partial_mod_k(const AttnArgs a, const AttnMod mod) {
  decode_attn_partial_body<KBITS, VBITS, NQ, true, true, true>(a, mod);
}

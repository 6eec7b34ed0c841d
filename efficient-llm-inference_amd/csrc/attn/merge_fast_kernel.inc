// merge_fast_kernel.inc — the text of the one-wave merge and of the one-round-trip merge, included twice by merge.inc: as
// merge_one_wave / decode_attn_merge_fast_k (KVQ_MERGE_PADDED 0: as they always were, token for token) and as merge_one_wave_padded /
// decode_attn_merge_fast_padded_k (KVQ_MERGE_PADDED 1: a left-padded batch: kv_start[b] is requested with everything else, the row's
// live splits follow from padded_lo as in its partial kernel, and a row that sees no key writes zeros instead of 0 / 0).
// ONE WAVE per query head (head_dim 128, at most 16 splits: what the LDS-staged kernel leaves): the same merge without the
// workgroup — lane s holds split s's (m, l), lane l holds d = l and d = 64 + l of every split's partial (32 loads, all
// requested before anything waits); the weights travel by v_readlane instead of an LDS table, and there is no barrier.
// The arithmetic, operand by operand and in the same order, is decode_attn_merge_fast_k's (its thread (g, d4) sums splits
// g, g + 8, the final row sums the 8 groups in order; its dot product sums d < 64 in wave 0 and d >= 64 in wave 1): equal bits.
// D = 64 (round 4: what the head_dim-64 ring kernel leaves): one element per lane, the block kernel's 16 split groups hold one
// split each (its dot product lives in wave 0 alone): the same chain with NH = 1.
// KVQ_MERGE_MOD 1 (merge_one_wave[_padded]_mod / decode_attn_merge_fast[_padded]_mod_k, the kvq_*_ex calls with a soft cap or
// sinks): the same texts with one more argument (AttnMod). The new token's score is soft-capped like the stored ones (the capped
// partial kernels did those), and the head's sink joins the merge as one more softmax term without a value row: M = max(M, sink),
// L += e^(sink - M), requested up front with everything else. The padded form of it reads a NULL kv_start as 0: it also serves
// the soft-capped calls without per-row starts, whose partial kernels are built from the padded texts.
#if KVQ_MERGE_PADDED && KVQ_MERGE_MOD
template <uint32_t D>
__device__ __forceinline__ void merge_one_wave_padded_mod(const AttnArgs& a, const bool has_new, const uint32_t hq, const uint32_t b, const AttnMod& mod) {
#elif KVQ_MERGE_PADDED
template <uint32_t D>
__device__ __forceinline__ void merge_one_wave_padded(const AttnArgs& a, const bool has_new, const uint32_t hq, const uint32_t b) {
#elif KVQ_MERGE_MOD
template <uint32_t D, bool RDEV = false>
__device__ __forceinline__ void merge_one_wave_mod(const AttnArgs& a, const bool has_new, const uint32_t hq, const uint32_t b, const AttnMod& mod) {
#else
template <uint32_t D, bool RDEV = false>
__device__ __forceinline__ void merge_one_wave(const AttnArgs& a, const bool has_new, const uint32_t hq, const uint32_t b) {
#endif
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  static_assert(D == 128 || D == 64, "head_dim of the one-wave merge");
  constexpr uint32_t G = 1024 / D, NSU = 16, NH = D / 64;  // the block kernel's split groups, splits held in registers, 64-element halves per lane
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t hk = hq / a.nq;
  const uint32_t nb = a.nsplit;  // 1 ... 16 (host)
  const float* ml = a.ws + ((int64_t)b * a.Hq + hq) * nb * 2;
  const float* src = a.ws + a.acc_off + ((int64_t)b * a.Hq + hq) * nb * D + lane;
  const uint32_t t_raw = (uint32_t)scalar_load_i32(a.t_dev ? a.t_dev : reinterpret_cast<const int*>(a.ws));
#if KVQ_MERGE_PADDED && KVQ_MERGE_MOD
  const int32_t ks_raw = a.kv_start ? kv_start_of(a, b) : 0;  // (a soft-capped call without per-row starts: every row starts at 0)
#elif KVQ_MERGE_PADDED
  const int32_t ks_raw = kv_start_of(a, b);  // this batch row's start: a scalar load, requested with everything else
#endif
#if KVQ_MERGE_MOD
  const float sink = mod.sinks ? mod.sinks[hq] : -INFINITY;  // this head's sink logit (a plain load: the array stays in L2 from step to step)
#endif
  const f32x2 ml_raw = __builtin_nontemporal_load(reinterpret_cast<const f32x2*>(ml) + (lane < nb ? lane : nb - 1u));
  uint16_t qraw[NH], kraw[NH], vraw[NH];
#pragma unroll
  for (int h = 0; h < (int)NH; ++h) {
    const uint32_t di = 64u * h + lane;
    qraw[h] = reinterpret_cast<const uint16_t*>(a.q)[(int64_t)b * a.q_sb + (int64_t)hq * a.q_sh + di];
    kraw[h] = reinterpret_cast<const uint16_t*>(a.kn)[(int64_t)b * a.kn_sb + (int64_t)hk * a.kn_sh + di];
    vraw[h] = reinterpret_cast<const uint16_t*>(a.vn)[(int64_t)b * a.vn_sb + (int64_t)hk * a.vn_sh + di];
  }
  float x[NH][NSU];
#pragma unroll
  for (int sp = 0; sp < (int)NSU; ++sp) {
    const uint32_t sc = (uint32_t)sp < nb ? (uint32_t)sp : nb - 1u;
#pragma unroll
    for (int h = 0; h < (int)NH; ++h) x[h][sp] = __builtin_nontemporal_load(src + (int64_t)sc * D + 64 * h);
  }
  __builtin_amdgcn_sched_barrier(0);
  const uint32_t T = a.t_dev ? (t_raw < a.T ? t_raw : a.T) : a.T;
#if KVQ_MERGE_PADDED
  uint32_t ns;
  {  // this batch row's live count and split size, as its partial kernel derived them (padded_lo)
    const uint32_t lt = T - padded_lo(a, T, ks_raw, has_new);
    const uint32_t ns_ts = padded_split_tokens(a, lt);
    ns = (lt + ns_ts - 1u) / ns_ts;
  }
#else
  uint32_t ns;
  if constexpr (RDEV) {  // the ring kernel under a device-side count chose its split size from that count (its own instantiation:
    // also every device-side count with a window; the host-count instantiation never evaluates window_lo)
    const uint32_t lt = T - window_lo(a, T);  // a sliding window: the visible stored tokens (the new-token slot stays T)
    const uint32_t ns_ts = live_split_tokens(a, lt);  // evaluated in the common one, even behind a branch, it cost the batch-1 call 0.3-0.7 us)
    ns = (lt + ns_ts - 1u) / ns_ts;
  } else {
    ns = a.t_dev ? (T + a.TS - 1u) / a.TS : nb;
  }
#endif
  ns = ns < nb ? ns : nb;
  f32x2 mlv = ml_raw;
  if (lane >= ns) mlv = f32x2{-INFINITY, 0.0f};
  auto widen = [&](uint16_t h) { return a.dtype == KVQ_F16 ? Elem<KVQ_F16>::widen(h) : Elem<KVQ_BF16>::widen(h); };
  const float p0 = wave_fsum(widen(has_new ? qraw[0] : (uint16_t)0) * widen(kraw[0]));
  float p1 = 0.0f;  // the block kernel's wave 1: d >= 64 (nothing at head_dim 64)
  if constexpr (NH == 2) p1 = wave_fsum(widen(has_new ? qraw[NH - 1] : (uint16_t)0) * widen(kraw[NH - 1]));
#if KVQ_MERGE_MOD
  const float s_tok = has_new ? softcap_score(((p0 + p1) + (0.0f + 0.0f)) * a.sm_scale, mod) : -INFINITY;
  const float M = fmaxf(fmaxf(wave_fmax(mlv[0]), s_tok), sink);
#else
  const float s_tok = has_new ? ((p0 + p1) + (0.0f + 0.0f)) * a.sm_scale : -INFINITY;
  const float M = fmaxf(wave_fmax(mlv[0]), s_tok);
#endif
  const float w = lane < ns ? __expf(mlv[0] - M) : 0.0f;
  const float lw = wave_fsum(lane < ns ? mlv[1] * w : 0.0f);
  const float w_new = has_new ? __expf(s_tok - M) : 0.0f;
#if KVQ_MERGE_MOD
  const float L = (((lw + 0.0f) + (0.0f + 0.0f)) + w_new) + (mod.sinks ? __expf(sink - M) : 0.0f);
#else
  const float L = ((lw + 0.0f) + (0.0f + 0.0f)) + w_new;
#endif
#if KVQ_MERGE_PADDED
  const float inv = L > 0.0f ? 1.0f / L : 0.0f;  // a row that sees no key (every split dead, no new token): zeros
#else
  const float inv = 1.0f / L;
#endif
  float wt[NSU];
#pragma unroll
  for (int sp = 0; sp < (int)NSU; ++sp) wt[sp] = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(w), sp));
#pragma unroll
  for (int h = 0; h < (int)NH; ++h) {
    float t = 0.0f;
#pragma unroll
    for (int k = 0; k < (int)G; ++k) {
      float o = 0.0f;
#pragma unroll
      for (int u = 0; u < (int)(NSU / G); ++u) {
        const int sp = k + u * (int)G;
        if ((uint32_t)sp < ns) o += x[h][sp] * wt[sp];
      }
      t += o;
    }
    if (has_new) t = fmaf(w_new, widen(vraw[h]), t);
    t *= inv;
    const int64_t oi = (int64_t)b * a.o_sb + (int64_t)hq * a.o_sh + 64 * h + lane;
    if (a.dtype == KVQ_F16) reinterpret_cast<f16*>(a.out)[oi] = (f16)t;
    else reinterpret_cast<__bf16*>(a.out)[oi] = (__bf16)t;
  }
}

// (has_new: without a new token the host points kn / vn at the query, so that the three loads need no branch)
// PF: partial rows each thread requests up front (and holds): ceil(nsplit / (256 / (D/4))) rounded up to 2 / 4 / 16 by the
// host — the 16 splits per head of the LDS-staged kernel need 2, not 16 (14 clamped re-reads of the last row per thread)
#if KVQ_MERGE_PADDED && KVQ_MERGE_MOD
template <int PF>
__global__ __launch_bounds__(kAttnBlock) void decode_attn_merge_fast_padded_mod_k(const AttnArgs a, const NewTokenArgs nt, const int fuse_quant_i,
                                                                                  const int has_new_i, const AttnMod mod) {
#elif KVQ_MERGE_PADDED
template <int PF>
__global__ __launch_bounds__(kAttnBlock) void decode_attn_merge_fast_padded_k(const AttnArgs a, const NewTokenArgs nt, const int fuse_quant_i,
                                                                              const int has_new_i) {
#elif KVQ_MERGE_MOD
template <int PF, bool RDEV = false>
__global__ __launch_bounds__(kAttnBlock) void decode_attn_merge_fast_mod_k(const AttnArgs a, const NewTokenArgs nt, const int fuse_quant_i,
                                                                           const int has_new_i, const AttnMod mod) {
#else
template <int PF, bool RDEV = false>
__global__ __launch_bounds__(kAttnBlock) void decode_attn_merge_fast_k(const AttnArgs a, const NewTokenArgs nt, const int fuse_quant_i,
                                                                       const int has_new_i) {
#endif
  __shared__ float s_red[3][kAttnBlock / kWave];
  // fuse_quant_i bit 0: the launch's last two workgroups quantise-append the new token; bit 1 (PF == 2, head_dim 128, <= 16
  // splits): ONE WAVE per head, four heads per workgroup (merge_one_wave)
  const int fuse_quant = fuse_quant_i & 1;
  const bool by_wave = PF == 2 && (fuse_quant_i & 2) != 0;
  const uint32_t n_head_wgs = by_wave ? (a.Hq + 3u) / 4u : a.Hq;
  if (blockIdx.x >= n_head_wgs) {  // new-token workgroups: (K | V) x pieces (one piece unless nt.nparts > 1)
    const uint32_t idx_new_tok = blockIdx.x - n_head_wgs, w_new_tok = idx_new_tok & 1u;
    if (fuse_quant && blockIdx.y == 0u && nt.nparts > 1u) {
      NewTokenArgs slot = nt;
      if (a.t_dev) {
        const int64_t T = (int64_t)live_tokens(a);
#pragma unroll
        for (int w = 0; w < 2; ++w) {
          slot.q[w] += T * nt.qs_t[w];
          slot.scale[w] += T;
        }
      }
      if (a.dtype == KVQ_F16) quant_new_token_parts<KVQ_F16>(slot, w_new_tok, idx_new_tok >> 1, s_red[0]);
      else quant_new_token_parts<KVQ_BF16>(slot, w_new_tok, idx_new_tok >> 1, s_red[0]);
    } else if (fuse_quant && blockIdx.y == 0u && new_token_fits_registers(nt, w_new_tok)) {
      if (a.dtype == KVQ_F16) quant_new_token_regs<KVQ_F16>(nt, w_new_tok, s_red[0], a.t_dev, a.T, a.q);
      else quant_new_token_regs<KVQ_BF16>(nt, w_new_tok, s_red[0], a.t_dev, a.T, a.q);
    } else if (fuse_quant && blockIdx.y == 0u) {
      NewTokenArgs slot = nt;
      if (a.t_dev) {
        const int64_t T = (int64_t)live_tokens(a);
#pragma unroll
        for (int w = 0; w < 2; ++w) {
          slot.q[w] += T * nt.qs_t[w];
          slot.scale[w] += T;
        }
      }
      if (a.dtype == KVQ_F16) quant_new_token_block<KVQ_F16>(slot, w_new_tok, s_red[0]);
      else quant_new_token_block<KVQ_BF16>(slot, w_new_tok, s_red[0]);
    }
    return;
  }
  if constexpr (PF == 2) {
    if (by_wave) {
      const uint32_t hq_w = blockIdx.x * 4u + (threadIdx.x >> 6);
      if (hq_w < a.Hq) {
#if KVQ_MERGE_PADDED && KVQ_MERGE_MOD
        if (a.D == 128u) merge_one_wave_padded_mod<128>(a, has_new_i != 0, hq_w, blockIdx.y, mod);
        else merge_one_wave_padded_mod<64>(a, has_new_i != 0, hq_w, blockIdx.y, mod);
#elif KVQ_MERGE_PADDED
        if (a.D == 128u) merge_one_wave_padded<128>(a, has_new_i != 0, hq_w, blockIdx.y);
        else merge_one_wave_padded<64>(a, has_new_i != 0, hq_w, blockIdx.y);
#elif KVQ_MERGE_MOD
        if (a.D == 128u) merge_one_wave_mod<128, RDEV>(a, has_new_i != 0, hq_w, blockIdx.y, mod);
        else merge_one_wave_mod<64, RDEV>(a, has_new_i != 0, hq_w, blockIdx.y, mod);
#else
        if (a.D == 128u) merge_one_wave<128, RDEV>(a, has_new_i != 0, hq_w, blockIdx.y);
        else merge_one_wave<64, RDEV>(a, has_new_i != 0, hq_w, blockIdx.y);
#endif
      }
      return;
    }
  }
  __shared__ float s_wt[kAttnBlock];
  __shared__ __attribute__((aligned(16))) float s_out[kAttnBlock * 4];
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const uint32_t tid = threadIdx.x;
  const uint32_t hq = blockIdx.x, b = blockIdx.y;
  const uint32_t hk = hq / a.nq;
  const bool has_new = has_new_i != 0;
  const uint32_t wave = tid >> 6, lane = tid & 63u;
  const uint32_t nb = a.nsplit;  // 1 ... kAttnBlock (host); the row stride of the partials
  const uint32_t dv = a.D >> 2;
  const uint32_t groups = kAttnBlock / dv;  // 32, 16, 8 or 4
  const uint32_t g = tid / dv, d4 = tid - g * dv;
  const float* ml = a.ws + ((int64_t)b * a.Hq + hq) * nb * 2;
  const f32x4* src = reinterpret_cast<const f32x4*>(a.ws + a.acc_off + ((int64_t)b * a.Hq + hq) * nb * a.D) + d4;

  // ---- requests: straight-line code (clamped indices, selected addresses), nothing waits before the fence -------
  // the device-side token count: a SCALAR buffer load (uniform address; a plain `*a.t_dev` becomes a vector load that is
  // waited for on the spot), issued here and waited for by the compiler at its first use below the fence
  const uint32_t t_raw = (uint32_t)scalar_load_i32(a.t_dev ? a.t_dev : reinterpret_cast<const int*>(a.ws));
#if KVQ_MERGE_PADDED && KVQ_MERGE_MOD
  const int32_t ks_raw = a.kv_start ? kv_start_of(a, b) : 0;  // (a soft-capped call without per-row starts: every row starts at 0)
#elif KVQ_MERGE_PADDED
  const int32_t ks_raw = kv_start_of(a, b);  // this batch row's start: a scalar load, requested with everything else
#endif
#if KVQ_MERGE_MOD
  const float sink = mod.sinks ? mod.sinks[hq] : -INFINITY;  // this head's sink logit (a plain load: the array stays in L2 from step to step)
#endif
  const f32x2 ml_raw = __builtin_nontemporal_load(reinterpret_cast<const f32x2*>(ml) + (tid < nb ? tid : nb - 1u));
  const uint32_t di = tid < a.D ? tid : a.D - 1u;
  const uint16_t qb_raw = reinterpret_cast<const uint16_t*>(a.q)[(int64_t)b * a.q_sb + (int64_t)hq * a.q_sh + di];
  const uint16_t kb = reinterpret_cast<const uint16_t*>(a.kn)[(int64_t)b * a.kn_sb + (int64_t)hk * a.kn_sh + di];
  const uint16_t vb = reinterpret_cast<const uint16_t*>(a.vn)[(int64_t)b * a.vn_sb + (int64_t)hk * a.vn_sh + di];
  f32x4 x[PF];
#pragma unroll
  for (int u = 0; u < PF; ++u) {
    const uint32_t s = g + (uint32_t)u * groups;
    x[u] = __builtin_nontemporal_load(src + (int64_t)(s < nb ? s : nb - 1u) * dv);
  }
  __builtin_amdgcn_sched_barrier(0);
  const uint32_t T = a.t_dev ? (t_raw < a.T ? t_raw : a.T) : a.T;
  const uint16_t qb = (has_new && tid < a.D) ? qb_raw : (uint16_t)0;  // the dot product runs over d < D
  f32x2 mlv = ml_raw;

  // ---- weights ---------------------------------------------------------------------------------------------
#if KVQ_MERGE_PADDED
  uint32_t ns;
  {  // this batch row's live count and split size, as its partial kernel derived them (padded_lo)
    const uint32_t lt = T - padded_lo(a, T, ks_raw, has_new);
    const uint32_t ns_ts = padded_split_tokens(a, lt);
    ns = (lt + ns_ts - 1u) / ns_ts;
  }
#else
  uint32_t ns;
  if constexpr (RDEV) {  // the ring kernel under a device-side count chose its split size from that count (its own instantiation:
    // also every device-side count with a window; the host-count instantiation never evaluates window_lo)
    const uint32_t lt = T - window_lo(a, T);  // a sliding window: the visible stored tokens (the new-token slot stays T)
    const uint32_t ns_ts = live_split_tokens(a, lt);  // evaluated in the common one, even behind a branch, it cost the batch-1 call 0.3-0.7 us)
    ns = (lt + ns_ts - 1u) / ns_ts;
  } else {
    ns = a.t_dev ? (T + a.TS - 1u) / a.TS : nb;
  }
#endif
  ns = ns < nb ? ns : nb;
  if (tid >= ns) mlv = f32x2{-INFINITY, 0.0f};
  auto widen = [&](uint16_t h) { return a.dtype == KVQ_F16 ? Elem<KVQ_F16>::widen(h) : Elem<KVQ_BF16>::widen(h); };
  {
    const float part = wave_fsum(widen(qb) * widen(kb));  // zero beyond D and without a new token
    const float mw = wave_fmax(mlv[0]);
    if (lane == 0u) {
      s_red[0][wave] = part;
      s_red[1][wave] = mw;
    }
  }
  lds_barrier();
#if KVQ_MERGE_MOD
  const float s_tok = has_new ? softcap_score(((s_red[0][0] + s_red[0][1]) + (s_red[0][2] + s_red[0][3])) * a.sm_scale, mod) : -INFINITY;
  const float M = fmaxf(fmaxf(fmaxf(fmaxf(s_red[1][0], s_red[1][1]), fmaxf(s_red[1][2], s_red[1][3])), s_tok), sink);
#else
  const float s_tok = has_new ? ((s_red[0][0] + s_red[0][1]) + (s_red[0][2] + s_red[0][3])) * a.sm_scale : -INFINITY;
  const float M = fmaxf(fmaxf(fmaxf(s_red[1][0], s_red[1][1]), fmaxf(s_red[1][2], s_red[1][3])), s_tok);
#endif
  {
    const float w = tid < ns ? __expf(mlv[0] - M) : 0.0f;
    s_wt[tid] = w;
    const float lw = wave_fsum(tid < ns ? mlv[1] * w : 0.0f);
    if (lane == 0u) s_red[2][wave] = lw;
  }
  lds_barrier();  // also publishes s_wt
  const float w_new = has_new ? __expf(s_tok - M) : 0.0f;
#if KVQ_MERGE_MOD
  const float L = (((s_red[2][0] + s_red[2][1]) + (s_red[2][2] + s_red[2][3])) + w_new) + (mod.sinks ? __expf(sink - M) : 0.0f);
#else
  const float L = ((s_red[2][0] + s_red[2][1]) + (s_red[2][2] + s_red[2][3])) + w_new;
#endif
#if KVQ_MERGE_PADDED
  const float inv = L > 0.0f ? 1.0f / L : 0.0f;  // a row that sees no key (every split dead, no new token): zeros
#else
  const float inv = 1.0f / L;
#endif

  // ---- weighted sum: thread = (split group g, 4 elements at d4) ---------------------------------------------
  f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int u = 0; u < PF; ++u) {
    const uint32_t s = g + (uint32_t)u * groups;
    if (s < ns) o += x[u] * s_wt[s];
  }
  for (uint32_t s = g + (uint32_t)PF * groups; s < ns; s += groups) o += src[(int64_t)s * dv] * s_wt[s];
  *reinterpret_cast<f32x4*>(&s_out[tid * 4]) = o;  // [g][d]
  lds_barrier();
  if (tid < a.D) {
    float t = 0.0f;
    for (uint32_t k = 0; k < groups; ++k) t += s_out[k * a.D + tid];
    if (has_new) t = fmaf(w_new, widen(vb), t);
    t *= inv;
    const int64_t oi = (int64_t)b * a.o_sb + (int64_t)hq * a.o_sh + tid;
    if (a.dtype == KVQ_F16) reinterpret_cast<f16*>(a.out)[oi] = (f16)t;
    else reinterpret_cast<__bf16*>(a.out)[oi] = (__bf16)t;
  }
}

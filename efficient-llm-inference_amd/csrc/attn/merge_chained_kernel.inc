// merge_chained_kernel.inc — the chained merge's text, included twice by merge.inc: as decode_attn_merge_k (KVQ_MERGE_PADDED 0: the
// kernel as it always was, token for token) and as decode_attn_merge_padded_k (KVQ_MERGE_PADDED 1: a left-padded batch, whose live
// splits are counted per batch row from padded_lo and whose rows without any visible key write zeros).
// One workgroup per (query head, batch row): log-sum-exp merge of the splits and of the exact new
// token. Split weights are computed once (one split per thread) and kept in LDS; the weighted sum
// runs 256 / D split groups wide with independent loads.
// With fuse_quant, two extra workgroups (blockIdx.x = Hq, Hq + 1 of batch row 0) quantise the new
// token's K / V into slot T of the stores (quant_new_token_block): nothing in this launch reads that
// slot, and the partial kernel that read [0, T) has finished, so a decode step is two launches.
// KVQ_MERGE_MOD 1 (decode_attn_merge_mod_k / decode_attn_merge_padded_mod_k, the kvq_*_ex calls with a soft cap or sinks): one more
// argument (AttnMod); the new token's score is soft-capped and the head's sink joins as one more softmax term without a value row
// (merge_fast_kernel.inc says the same of its two bodies). The padded form of it reads a NULL kv_start as 0.
#if KVQ_MERGE_PADDED && KVQ_MERGE_MOD
__global__ __launch_bounds__(kAttnBlock) void decode_attn_merge_padded_mod_k(const AttnArgs a, const NewTokenArgs nt, const int fuse_quant, const AttnMod mod) {
#elif KVQ_MERGE_PADDED
__global__ __launch_bounds__(kAttnBlock) void decode_attn_merge_padded_k(const AttnArgs a, const NewTokenArgs nt, const int fuse_quant) {
#elif KVQ_MERGE_MOD
__global__ __launch_bounds__(kAttnBlock) void decode_attn_merge_mod_k(const AttnArgs a, const NewTokenArgs nt, const int fuse_quant, const AttnMod mod) {
#else
__global__ __launch_bounds__(kAttnBlock) void decode_attn_merge_k(const AttnArgs a, const NewTokenArgs nt, const int fuse_quant) {
#endif
  __shared__ float s_red[kAttnBlock / kWave];
  if (blockIdx.x >= a.Hq) {  // new-token workgroups: (K | V) x pieces (one piece unless nt.nparts > 1)
    if (fuse_quant && blockIdx.y == 0u) {
      const uint32_t idx = blockIdx.x - a.Hq, wkv = idx & 1u, part = idx >> 1;
      NewTokenArgs slot = nt;
      if (a.t_dev) {  // the host passed slot 0; the real slot is the device-side T
        const int64_t T = (int64_t)live_tokens(a);
#pragma unroll
        for (int w = 0; w < 2; ++w) {
          slot.q[w] += T * nt.qs_t[w];
          slot.scale[w] += T;
        }
      }
      if (nt.nparts > 1u) {
        if (a.dtype == KVQ_F16) quant_new_token_parts<KVQ_F16>(slot, wkv, part, s_red);
        else quant_new_token_parts<KVQ_BF16>(slot, wkv, part, s_red);
      } else if (a.dtype == KVQ_F16) quant_new_token_block<KVQ_F16>(slot, wkv, s_red);
      else quant_new_token_block<KVQ_BF16>(slot, wkv, s_red);
    }
    return;
  }
  __shared__ float s_wt[kAttnMaxSplit];
  __shared__ __attribute__((aligned(16))) float s_out[kAttnBlock * 4];
  const uint32_t tid = threadIdx.x;
  const uint32_t hq = blockIdx.x, b = blockIdx.y;
  const uint32_t hk = hq / a.nq;
  const bool has_new = a.kn != nullptr;
  const uint32_t wave = tid >> 6, lane = tid & 63u;
  auto block_reduce = [&](float v, bool is_max) -> float {
    v = is_max ? wave_fmax(v) : wave_fsum(v);
    __syncthreads();  // s_red free again
    if (lane == 0u) s_red[wave] = v;
    __syncthreads();
    return is_max ? fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3])) : (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
  };
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  float s_tok = -INFINITY;
  if (has_new) {
    float part = 0.0f;
    for (uint32_t d = tid; d < a.D; d += kAttnBlock)
      part += load_elem(a.q, (int64_t)b * a.q_sb + (int64_t)hq * a.q_sh + d, a.dtype) *
              load_elem(a.kn, (int64_t)b * a.kn_sb + (int64_t)hk * a.kn_sh + d, a.dtype);
    s_tok = block_reduce(part, false) * a.sm_scale;
#if KVQ_MERGE_MOD
    s_tok = softcap_score(s_tok, mod);
#endif
  }
  const float* ml = a.ws + ((int64_t)b * a.Hq + hq) * a.nsplit * 2;
  const float* accb = a.ws + a.acc_off + ((int64_t)b * a.Hq + hq) * a.nsplit * a.D;
  // a.nsplit is the row stride of the partials; with a device-side T only the first ceil(T / TS) are live
#if KVQ_MERGE_PADDED
  uint32_t ns;
  {  // this batch row's live splits: the count its partial kernel derived (padded_lo)
#if KVQ_MERGE_MOD
    // (a soft-capped call without per-row starts: every row starts at 0)
    const uint32_t t = live_tokens(a), lt = t - padded_lo(a, t, a.kv_start ? kv_start_of(a, b) : 0, has_new), ns_ts = padded_split_tokens(a, lt);
#else
    const uint32_t t = live_tokens(a), lt = t - padded_lo(a, t, kv_start_of(a, b), has_new), ns_ts = padded_split_tokens(a, lt);
#endif
    ns = (lt + ns_ts - 1u) / ns_ts;
    ns = ns < a.nsplit ? ns : a.nsplit;
  }
#else
  uint32_t ns = a.nsplit;
  if (a.t_dev) {  // (kept out of the host-count path: evaluated there it cost the batch-1 call 0.7 us)
    const uint32_t t = live_tokens(a), lt = t - window_lo(a, t), ns_ts = live_split_tokens(a, lt);
    ns = (lt + ns_ts - 1u) / ns_ts;
  }
#endif
  // this thread's splits: tid, tid + 256, ...; (m, l) is read twice (second time from cache) rather
  // than kept in a register array sized for kAttnMaxSplit
#if KVQ_MERGE_MOD
  const float sink = mod.sinks ? mod.sinks[hq] : -INFINITY;  // this head's sink logit
  float m_max = fmaxf(s_tok, sink);
#else
  float m_max = s_tok;
#endif
  for (uint32_t s = tid; s < ns; s += kAttnBlock) m_max = fmaxf(m_max, ml[2 * s]);
  const float M = block_reduce(m_max, true);
  float lsum = 0.0f;
  for (uint32_t s = tid; s < ns; s += kAttnBlock) {
    const float w = __expf(ml[2 * s] - M);
    s_wt[s] = w;
    lsum += ml[2 * s + 1] * w;
  }
  const float w_new = has_new ? __expf(s_tok - M) : 0.0f;
#if KVQ_MERGE_MOD
  const float L = (block_reduce(lsum, false) + w_new) + (mod.sinks ? __expf(sink - M) : 0.0f);  // the barriers inside also publish s_wt
#else
  const float L = block_reduce(lsum, false) + w_new;  // the barriers inside also publish s_wt
#endif
#if KVQ_MERGE_PADDED
  const float inv = L > 0.0f ? 1.0f / L : 0.0f;  // a row that sees no key (every split dead, no new token): zeros
#else
  const float inv = 1.0f / L;
#endif
  // weighted sum, 16 bytes per lane: thread = (split group g, 4 elements at d4); 1024 / D groups.
  // (Requesting the first 8 rows + the new-token operands before the reductions measured slower:
  // 7.6 vs 5.1 us at 128 splits.)
  const uint32_t dv = a.D >> 2;
  const uint32_t groups = kAttnBlock / dv;  // 32, 16, 8 or 4
  const uint32_t g = tid / dv, d4 = tid - g * dv;
  f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
  {
    const f32x4* src = reinterpret_cast<const f32x4*>(accb) + d4;
    uint32_t s = g;
    for (; s + 7u * groups < ns; s += 8u * groups) {  // 8 independent loads in flight: at batch 1 the merge is pure latency
      f32x4 x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = src[(int64_t)(s + (uint32_t)u * groups) * dv];
#pragma unroll
      for (int u = 0; u < 8; ++u) o += x[u] * s_wt[s + (uint32_t)u * groups];
    }
    for (; s + 3u * groups < ns; s += 4u * groups) {  // 4 independent loads in flight
      const f32x4 x0 = src[(int64_t)s * dv];
      const f32x4 x1 = src[(int64_t)(s + groups) * dv];
      const f32x4 x2 = src[(int64_t)(s + 2u * groups) * dv];
      const f32x4 x3 = src[(int64_t)(s + 3u * groups) * dv];
      o += x0 * s_wt[s] + x1 * s_wt[s + groups] + x2 * s_wt[s + 2u * groups] + x3 * s_wt[s + 3u * groups];
    }
    for (; s < ns; s += groups) o += src[(int64_t)s * dv] * s_wt[s];
  }
  *reinterpret_cast<f32x4*>(&s_out[tid * 4]) = o;  // [g][d]
  __syncthreads();
  if (tid < a.D) {
    float t = 0.0f;
    for (uint32_t k = 0; k < groups; ++k) t += s_out[k * a.D + tid];
    if (has_new) t = fmaf(w_new, load_elem(a.vn, (int64_t)b * a.vn_sb + (int64_t)hk * a.vn_sh + tid, a.dtype), t);
    t *= inv;
    const int64_t oi = (int64_t)b * a.o_sb + (int64_t)hq * a.o_sh + tid;
    if (a.dtype == KVQ_F16) reinterpret_cast<f16*>(a.out)[oi] = (f16)t;
    else reinterpret_cast<__bf16*>(a.out)[oi] = (__bf16)t;
  }
}


// host.inc — part of kvq_attn.hip (one translation unit, included in this order): plans (which kernel, how many splits), launchers and the extern "C" entry points
constexpr int64_t kLdsSlots = 256 * 4;  // one-wave workgroups of the LDS-staged kernel resident at once (4 per CU)

// tokens per workgroup: one loop iteration (D/16 lanes per token, kAttnUnroll tokens per lane) while
// the grid stays below ~4096 workgroups, whole multiples of it beyond; never more than
// kAttnMaxSplit splits
static bool use_mfma(const kvq_attn_dims_t* d) {
  const int64_t nq = d->Hkv > 0 ? d->Hq / d->Hkv : 0;
  // every grouping from 1 query head per kv head on (round 4: the MFMA kernels beat the VALU kernel at 1 per kv head too —
  // Llama-2-7B batch 8 41.0 -> 39.0 us per layer call on the ring kernel, gpt2 at 1,024 tokens 9.9 -> 8.1 us on the one-tile
  // kernel, profiles/r04f_*; rounds 1-3 drew the line at 3)
  return (d->D == 128 || d->D == 64) && nq >= 1 && nq <= 16 && !tunables().attn_force_valu;
}
// LDS-staged streaming kernel (the ring kernel: contiguous 1 KiB requests into an LDS ring), the only streaming kernel:
// head_dim 128, and head_dim 64 with INT8 keys (k_bits; sizing calls pass 8 and cover the one-tile plan beside it).
// attn_lds: -1 (default) / 1 = it serves every streaming plan; 0 = never (one-tile splits instead).
static bool use_lds(const kvq_attn_dims_t* d, int k_bits = 8) {
  return tunables().attn_lds != 0 && use_mfma(d) && (d->D == 128 || (d->D == 64 && k_bits == 8));
}
constexpr int kStreamTC = 64;  // tokens per tile of the ring kernel
// ring kernel: tiles per wave (0 = one-tile splits). Chosen so that every wave of the launch is resident at once (one
// round) when the batch offers more 64-token tiles than the chip has wave slots.
static uint32_t stream_tpw(const kvq_attn_dims_t* d, int k_bits = 8) {
  if (!use_lds(d, k_bits) || d->T <= 0) return 0;
  const int64_t forced = tunables().attn_stream_tpw;  // -1 = never, 0 = by size, > 0 = that many
  if (forced < 0) return 0;
  const int64_t ntiles = (d->T + kStreamTC - 1) / kStreamTC;
  // wave slots of one round: the ring kernel holds its tiles in LDS, 4 one-wave workgroups per CU (head_dim 64 too:
  // 2048 slots measured 24.9 us per call against 23.7 at 1024, Llama-3.2-1B batch 8)
  int64_t tpw = forced > 0 ? forced : (ntiles * d->B * d->Hkv + kLdsSlots - 1) / kLdsSlots;
  // by size: the ring pays from three tiles per wave on (batch 1 at 16 K tokens = two tiles per wave: 14.9 us per layer
  // call against 13.7 for one-tile splits)
  if (forced <= 0 && tpw < 3) return 0;
  if (tpw > ntiles) tpw = ntiles;
  return (uint32_t)tpw;
}
static bool plan_onetile(const kvq_attn_dims_t* d, uint32_t* ts, uint32_t* nsplit);
// tpw_out (optional): tiles per wave of the streaming layout when THAT is what the plan chose, 0 when it fell back to
// one-tile splits (the launcher must size its kernel choice from this, never from stream_tpw() on its own)
static bool plan(const kvq_attn_dims_t* d, uint32_t* ts, uint32_t* nsplit, uint32_t* tpw_out = nullptr, int k_bits = 8) {
  if (tpw_out) *tpw_out = 0;
  if (const uint32_t tpw = stream_tpw(d, k_bits)) {  // one wave per tpw tiles of 64 tokens
    const int64_t per = (int64_t)tpw * kStreamTC;
    *ts = (uint32_t)per;
    *nsplit = (uint32_t)((d->T + per - 1) / per);
    if (*nsplit <= (uint32_t)kAttnMaxSplit) {
      if (tpw_out) *tpw_out = tpw;
      return true;
    }
  }
  return plan_onetile(d, ts, nsplit);
}
// one tile (MFMA kernel) / one workgroup pass (VALU kernel) per split: also the only shapes a device-side T takes
static bool plan_onetile(const kvq_attn_dims_t* d, uint32_t* ts, uint32_t* nsplit) {
  if (use_mfma(d)) {  // one wave per split of TC tokens
    const int64_t tc = kAttnMfmaTC;
    *ts = (uint32_t)tc;
    *nsplit = (uint32_t)((d->T + tc - 1) / tc);
    return *nsplit <= (uint32_t)kAttnMaxSplit;
  }
  const int64_t step = (int64_t)(kAttnBlock / (d->D / 16)) * kAttnUnroll;
  const int64_t bh = d->B * d->Hkv > 0 ? d->B * d->Hkv : 1;
  int64_t m = (d->T * bh + step * 4096 - 1) / (step * 4096);
  if (m < 1) m = 1;
  int64_t per = m * step;
  if (per > kAttnMaxTS) per = kAttnMaxTS / step * step;
  if ((d->T + per - 1) / per > kAttnMaxSplit) per = kAttnMaxTS / step * step;
  *ts = (uint32_t)per;
  *nsplit = (uint32_t)((d->T + per - 1) / per);
  return *nsplit <= (uint32_t)kAttnMaxSplit;
}

// The workspace starts with one word per (batch row, kv head), padded to 16 bytes, in front of the partials: room for the
// arrival tickets of an in-launch merge that measured slower (r04b). Nothing uses them; the layout stays as it was.
static int64_t arrive_floats(const kvq_attn_dims_t* d) { return (d->B * d->Hkv + 3) / 4 * 4; }

// The partial launch of a left-padded batch (a.arrive = kv_start): the same routes as launch_partial, each in its padded
// instantiation (per-row lo on the device), for a host count and a device count alike.
template <int KBITS, int VBITS>
static void launch_partial_padded(const AttnArgs& a, hipStream_t st) {
  const dim3 grid(a.nsplit, a.Hkv, a.B);
  constexpr bool kI8 = KBITS == 8;
  if constexpr (kI8) {
    if (a.mfma && a.stream_tpw && a.lds == 1u && a.D == 64u) {
      constexpr int kSlot64 = 64 * (64 * KBITS / 8 + 64 * VBITS / 8) + 512;
      if (a.nq <= 4u) KVQ_LAUNCH((decode_attn_lds_mfma_padded_k<KBITS, VBITS, 64, kI8, 2, 4, 64>), grid, dim3(kWave), (size_t)(2 * kSlot64), st, a, a.stream_tpw);
      else KVQ_LAUNCH((decode_attn_lds_mfma_padded_k<KBITS, VBITS, 64, kI8, 2, 1, 64>), grid, dim3(kWave), (size_t)(2 * kSlot64), st, a, a.stream_tpw);
      return;
    }
  }
  if (a.mfma && a.stream_tpw && a.lds && a.D == 128u) {
    constexpr int kSlot = 64 * (128 * KBITS / 8 + 128 * VBITS / 8) + 512;
    if constexpr (kI8) {
      if (a.nq <= 4u) {
        KVQ_LAUNCH((decode_attn_lds_mfma_padded_k<KBITS, VBITS, 64, kI8, 2, 4, 128>), grid, dim3(kWave), (size_t)(2 * kSlot), st, a, a.stream_tpw);
        return;
      }
    }
    KVQ_LAUNCH((decode_attn_lds_mfma_padded_k<KBITS, VBITS, 64, kI8, 2, 1, 128>), grid, dim3(kWave), (size_t)(2 * kSlot), st, a, a.stream_tpw);
    return;
  }
  if (a.mfma) {
    if (a.D == 64u) KVQ_LAUNCH((decode_attn_partial_mfma_padded_k<KBITS, VBITS, kAttnMfmaTC, 64>), grid, dim3(kWave), 0, st, a);
    else KVQ_LAUNCH((decode_attn_partial_mfma_padded_k<KBITS, VBITS, kAttnMfmaTC, 128>), grid, dim3(kWave), 0, st, a);
    return;
  }
  if (a.nq == 1) KVQ_LAUNCH((decode_attn_partial_padded_k<KBITS, VBITS, 1>), grid, dim3(kAttnBlock), 0, st, a);
  else if (a.nq == 2) KVQ_LAUNCH((decode_attn_partial_padded_k<KBITS, VBITS, 2>), grid, dim3(kAttnBlock), 0, st, a);
  else if (a.nq <= 4) KVQ_LAUNCH((decode_attn_partial_padded_k<KBITS, VBITS, 4>), grid, dim3(kAttnBlock), 0, st, a);
  else KVQ_LAUNCH((decode_attn_partial_padded_k<KBITS, VBITS, 8>), grid, dim3(kAttnBlock), 0, st, a);
}

template <int KBITS, int VBITS>
static void launch_partial(const AttnArgs& a, hipStream_t st) {
  const dim3 grid(a.nsplit, a.Hkv, a.B);
  // INT8 keys at head_dim 128 in the streaming kernel: the stored bytes straight into the int8 MFMA, the query as two
  // int8 planes whose cost is amortised over the wave's tiles (50.6 vs 52.3 us per call at batch 8).
  constexpr bool kI8 = KBITS == 8;
  if constexpr (kI8) {
    if (a.mfma && a.stream_tpw && a.lds == 1u && a.D == 64u) {  // head_dim 64 (INT8 keys): ring depth 2, eight one-wave workgroups per CU
      constexpr int kSlot64 = 64 * (64 * KBITS / 8 + 64 * VBITS / 8) + 512;
      if (a.t_dev) {  // a device-side count: the instantiation whose waves take their tile range from it
        if (a.nq <= 4u) KVQ_LAUNCH((decode_attn_lds_mfma_k<KBITS, VBITS, 64, kI8, 2, 4, 64, true>), grid, dim3(kWave), (size_t)(2 * kSlot64), st, a, a.stream_tpw);
        else KVQ_LAUNCH((decode_attn_lds_mfma_k<KBITS, VBITS, 64, kI8, 2, 1, 64, true>), grid, dim3(kWave), (size_t)(2 * kSlot64), st, a, a.stream_tpw);
      } else if (a.nq <= 4u) KVQ_LAUNCH((decode_attn_lds_mfma_k<KBITS, VBITS, 64, kI8, 2, 4, 64>), grid, dim3(kWave), (size_t)(2 * kSlot64), st, a, a.stream_tpw);
      else KVQ_LAUNCH((decode_attn_lds_mfma_k<KBITS, VBITS, 64, kI8, 2, 1, 64>), grid, dim3(kWave), (size_t)(2 * kSlot64), st, a, a.stream_tpw);
      return;
    }
  }
  if (a.mfma && a.stream_tpw && a.lds && a.D == 128u) {
    // ring depth 2: one tile in flight behind the one being reduced, four one-wave workgroups per CU (25.6 KiB each for
    // INT8 keys + INT4 values). Measured at batch 8, 16 K tokens (per layer call incl. merge, profiles/r03d_*): depth 2
    // 40.8 us, depth 3 44.7 us, depth 4 (three workgroups per CU) 86 us; 32-token tiles 42.1-51.6 us.
    constexpr int kSlot = 64 * (128 * KBITS / 8 + 128 * VBITS / 8) + 512;
    if constexpr (kI8) {  // at most 4 query heads per kv head: one score output per tile (AttnStream TG = 4)
      if (a.nq <= 4u) {
        if (a.t_dev) KVQ_LAUNCH((decode_attn_lds_mfma_k<KBITS, VBITS, 64, kI8, 2, 4, 128, true>), grid, dim3(kWave), (size_t)(2 * kSlot), st, a, a.stream_tpw);  // device-side count
        else KVQ_LAUNCH((decode_attn_lds_mfma_k<KBITS, VBITS, 64, kI8, 2, 4>), grid, dim3(kWave), (size_t)(2 * kSlot), st, a, a.stream_tpw);
        return;
      }
    }
    if (a.t_dev) KVQ_LAUNCH((decode_attn_lds_mfma_k<KBITS, VBITS, 64, kI8, 2, 1, 128, true>), grid, dim3(kWave), (size_t)(2 * kSlot), st, a, a.stream_tpw);  // device-side count
    else KVQ_LAUNCH((decode_attn_lds_mfma_k<KBITS, VBITS, 64, kI8, 2>), grid, dim3(kWave), (size_t)(2 * kSlot), st, a, a.stream_tpw);
    return;
  }
  // a device-side count under a window: the one-tile kernels' own instantiations (the host-count ones never evaluate it)
  const bool win = a.t_dev && a.window > 0;
  if (a.mfma) {
    if (win) {
      if (a.D == 64u) KVQ_LAUNCH((decode_attn_partial_mfma_window_k<KBITS, VBITS, kAttnMfmaTC, 64>), grid, dim3(kWave), 0, st, a);
      else KVQ_LAUNCH((decode_attn_partial_mfma_window_k<KBITS, VBITS, kAttnMfmaTC, 128>), grid, dim3(kWave), 0, st, a);
    } else if (a.D == 64u) KVQ_LAUNCH((decode_attn_partial_mfma_k<KBITS, VBITS, kAttnMfmaTC, 64>), grid, dim3(kWave), 0, st, a);
    else KVQ_LAUNCH((decode_attn_partial_mfma_k<KBITS, VBITS, kAttnMfmaTC, 128>), grid, dim3(kWave), 0, st, a);
    return;
  }
  if (win) {
    if (a.nq == 1) KVQ_LAUNCH((decode_attn_partial_window_k<KBITS, VBITS, 1>), grid, dim3(kAttnBlock), 0, st, a);
    else if (a.nq == 2) KVQ_LAUNCH((decode_attn_partial_window_k<KBITS, VBITS, 2>), grid, dim3(kAttnBlock), 0, st, a);
    else if (a.nq <= 4) KVQ_LAUNCH((decode_attn_partial_window_k<KBITS, VBITS, 4>), grid, dim3(kAttnBlock), 0, st, a);
    else KVQ_LAUNCH((decode_attn_partial_window_k<KBITS, VBITS, 8>), grid, dim3(kAttnBlock), 0, st, a);
    return;
  }
  if (a.nq == 1) KVQ_LAUNCH((decode_attn_partial_k<KBITS, VBITS, 1>), grid, dim3(kAttnBlock), 0, st, a);
  else if (a.nq == 2) KVQ_LAUNCH((decode_attn_partial_k<KBITS, VBITS, 2>), grid, dim3(kAttnBlock), 0, st, a);
  else if (a.nq <= 4) KVQ_LAUNCH((decode_attn_partial_k<KBITS, VBITS, 4>), grid, dim3(kAttnBlock), 0, st, a);
  else KVQ_LAUNCH((decode_attn_partial_k<KBITS, VBITS, 8>), grid, dim3(kAttnBlock), 0, st, a);
}

}  // namespace kvq

using namespace kvq;

extern "C" {

int64_t kvq_decode_attn_workspace(const kvq_attn_dims_t* d) {
  if (!d || d->B <= 0 || d->Hq <= 0 || d->Hkv <= 0 || d->T < 0 || d->D <= 0) return -1;
  if (d->D != 32 && d->D != 64 && d->D != 128 && d->D != 256) return -1;
  uint32_t ts, ns, ns1;
  if (!plan(d, &ts, &ns)) return -1;
  // kvq_decode_step_dev always takes one-tile splits, which can be more than the streaming layout's: cover both
  if (plan_onetile(d, &ts, &ns1) && ns1 > ns) ns = ns1;
  const int64_t rows = d->B * d->Hq * (int64_t)(ns > 0 ? ns : 1);
  const int64_t legacy = (rows * 2 + 3) / 4 * 4 + rows * d->D;
  return arrive_floats(d) + legacy;
}

}  // extern "C"

// shared body of kvq_decode_attn / kvq_decode_step; nt != nullptr: quantise the new token in the merge launch
static int decode_attn_impl(const char* name, const void* q, int64_t q_sb, int64_t q_sh, const uint8_t* k_store,
                            const kvq_strides_t* k_st, const float* k_scales, int k_bits, const uint8_t* v_store,
                            const kvq_strides_t* v_st, const float* v_scales, int v_bits, const void* k_new,
                            int64_t kn_sb, int64_t kn_sh, const void* v_new, int64_t vn_sb, int64_t vn_sh, void* out,
                            int64_t o_sb, int64_t o_sh, int dtype, float sm_scale, float* workspace,
                            int64_t workspace_floats, const kvq_attn_dims_t* d, void* stream, const NewTokenArgs* nt,
                            const int32_t* t_dev = nullptr, const int64_t window = 0, const int32_t* kv_start = nullptr) {
  if (!d || !q || !out) {
    set_error("%s: NULL q / out / dims", name);
    return KVQ_E_NULL;
  }
  if (const int rcd = check_device(out, name)) return rcd;
  if (kv_start) {
    if (const int rcd = check_device(kv_start, name)) return rcd;
  }
  if (d->B <= 0 || d->Hq <= 0 || d->Hkv <= 0 || d->T < 0 || d->B >= (1 << 16) || d->Hkv >= (1 << 16) ||
      d->T >= (int64_t(1) << 31) || d->Hq % d->Hkv != 0 || d->Hq / d->Hkv > (use_mfma(d) ? 16 : 8)) {
    set_error("%s: bad dims B=%lld Hq=%lld Hkv=%lld T=%lld (need Hq %% Hkv == 0, Hq / Hkv <= 8, or <= 16 at head_dim 64 / 128)", name, (long long)d->B,
              (long long)d->Hq, (long long)d->Hkv, (long long)d->T);
    return KVQ_E_DIMS;
  }
  if (d->D != 32 && d->D != 64 && d->D != 128 && d->D != 256) {
    set_error("%s: head_dim %lld not supported (32, 64, 128, 256)", name, (long long)d->D);
    return KVQ_E_DIMS;
  }
  if (dtype != KVQ_F16 && dtype != KVQ_BF16) {
    set_error("%s: dtype %d not supported (KVQ_F16, KVQ_BF16)", name, dtype);
    return KVQ_E_DTYPE;
  }
  if ((k_bits != 8 && k_bits != 4) || (v_bits != 8 && v_bits != 4)) {
    set_error("%s: k_bits / v_bits must be 8 or 4", name);
    return KVQ_E_DIMS;
  }
  if ((k_new == nullptr) != (v_new == nullptr)) {
    set_error("%s: k_new and v_new must be given together", name);
    return KVQ_E_NULL;
  }
  if (d->T == 0 && !k_new) {
    set_error("%s: nothing to attend to (T == 0 and no new token)", name);
    return KVQ_E_DIMS;
  }
  if (d->T > 0 && (!k_store || !v_store || !k_scales || !v_scales || !k_st || !v_st || !workspace)) {
    set_error("%s: NULL store / scales / strides / workspace", name);
    return KVQ_E_NULL;
  }
  // A device-side count under a window attends at most W - 1 stored tokens whatever the count: the grid and the split layout
  // are planned for that (pd), while a.T stays the caller's bound (the clamp of the count and of the new-token slot).
  kvq_attn_dims_t dp = *d;
  if (t_dev && window > 0 && window - 1 < d->T) dp.T = window - 1;
  // A padded call, host count or device count: per-row starts live on the device, so the grid is planned for what the window
  // alone leaves visible (W keys with the query's own: W - 1 stored ones beside a new token, W without one)
  if (kv_start && window > 0 && window - (k_new ? 1 : 0) < d->T) dp.T = window - (k_new ? 1 : 0);
  const kvq_attn_dims_t* pd = &dp;
  const int64_t need = kvq_decode_attn_workspace(pd);
  if (d->T > 0 && workspace_floats < need) {
    set_error("%s: workspace of %lld floats, %lld needed", name, (long long)workspace_floats, (long long)need);
    return KVQ_E_DIMS;
  }
  const int kal = k_bits == 8 ? 16 : 8, val = v_bits == 8 ? 16 : 8;
  if (d->T > 0 && (!aligned(k_store, kal) || k_st->b % kal || k_st->h % kal || k_st->t % kal || !aligned(v_store, val) ||
                   v_st->b % val || v_st->h % val || v_st->t % val)) {
    set_error("%s: store rows must be %d / %d byte aligned", name, kal, val);
    return KVQ_E_DIMS;
  }
  if (d->T > 0 && (d->T * k_st->t >= (int64_t(1) << 31) || d->T * v_st->t >= (int64_t(1) << 31))) {
    set_error("%s: one (batch, kv head) row of the store must stay below 2 GiB", name);
    return KVQ_E_DIMS;
  }
  if (!aligned(q, 16) || q_sb % 8 || q_sh % 8) {
    set_error("%s: q must be 16-byte aligned with strides that are multiples of 8 elements", name);
    return KVQ_E_DIMS;
  }
  AttnArgs a;
  a.q = q; a.q_sb = q_sb; a.q_sh = q_sh;
  a.k = k_store; a.v = v_store;
  if (d->T > 0) {
    a.k_sb = k_st->b; a.k_sh = k_st->h; a.k_st = k_st->t;
    a.v_sb = v_st->b; a.v_sh = v_st->h; a.v_st = v_st->t;
  } else {
    a.k_sb = a.k_sh = a.k_st = a.v_sb = a.v_sh = a.v_st = 0;
  }
  a.k_scale = k_scales; a.v_scale = v_scales;
  a.kn = k_new; a.kn_sb = kn_sb; a.kn_sh = kn_sh;
  a.vn = v_new; a.vn_sb = vn_sb; a.vn_sh = vn_sh;
  a.out = out; a.o_sb = o_sb; a.o_sh = o_sh;
  const int64_t arrive_n = arrive_floats(d);
  a.ws = workspace ? workspace + arrive_n : workspace;
  workspace_floats -= arrive_n;
  a.arrive = reinterpret_cast<uint32_t*>(const_cast<int32_t*>(kv_start));  // read by the *_padded_k kernels only
  a.ws_bytes = 0u;
  a.window = (t_dev || kv_start) ? (int32_t)(window < INT32_MAX ? window : INT32_MAX) : 0;
  a.sm_scale = sm_scale;
  a.B = (uint32_t)d->B; a.Hq = (uint32_t)d->Hq; a.Hkv = (uint32_t)d->Hkv; a.T = (uint32_t)d->T; a.D = (uint32_t)d->D;
  a.nq = (uint32_t)(d->Hq / d->Hkv);
  a.lpt_shift = ilog2_exact(d->D / 16);
  a.dtype = dtype;
  a.mfma = use_mfma(d) ? 1 : 0;
  a.stream_tpw = 0u;
  // a device-side count (graph replay) takes the ring kernel too — its waves spread the live tiles over the launch (ring_dev_tpw) —
  // unless the knob says one-tile splits as before (attn_ring_dev = 0)
  const bool ring_dev = t_dev && tunables().attn_ring_dev != 0;
  a.lds = ((!t_dev || ring_dev) && use_lds(pd, k_bits)) ? 1u : 0u;
  a.t_dev = t_dev;
  if (!((t_dev && !ring_dev) ? plan_onetile(pd, &a.TS, &a.nsplit) : plan(pd, &a.TS, &a.nsplit, &a.stream_tpw, k_bits))) {
    set_error("%s: T=%lld needs more than %d splits of %d tokens", name, (long long)d->T, kAttnMaxSplit, kAttnMaxTS);
    return KVQ_E_DIMS;
  }
  a.acc_off = ((int64_t)a.B * a.Hq * a.nsplit * 2 + 3) / 4 * 4;
  // the split layout actually chosen (a device-side T always takes one-tile splits) must fit too
  if (d->T > 0 && workspace_floats < a.acc_off + (int64_t)a.B * a.Hq * a.nsplit * a.D) {
    set_error("%s: workspace of %lld floats, %lld needed for %u splits", name, (long long)workspace_floats,
              (long long)(a.acc_off + (int64_t)a.B * a.Hq * a.nsplit * a.D), a.nsplit);
    return KVQ_E_DIMS;
  }
  if (d->T > 0 && !aligned(workspace, 16)) {
    set_error("%s: workspace must be 16-byte aligned", name);
    return KVQ_E_DIMS;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (a.nsplit > 0 && kv_start) {
    if (k_bits == 8 && v_bits == 8) launch_partial_padded<8, 8>(a, st);
    else if (k_bits == 8) launch_partial_padded<8, 4>(a, st);
    else if (v_bits == 8) launch_partial_padded<4, 8>(a, st);
    else launch_partial_padded<4, 4>(a, st);
    const int rc = check_launch(name);
    if (rc) return rc;
  } else if (a.nsplit > 0) {
    if (k_bits == 8 && v_bits == 8) launch_partial<8, 8>(a, st);
    else if (k_bits == 8) launch_partial<8, 4>(a, st);
    else if (v_bits == 8) launch_partial<4, 8>(a, st);
    else launch_partial<4, 4>(a, st);
    const int rc = check_launch(name);
    if (rc) return rc;
  }
  NewTokenArgs none = {};
  if (a.nsplit >= 1u && a.nsplit <= (uint32_t)kAttnBlock && a.D <= (uint32_t)kAttnBlock && tunables().attn_merge_fast)
  {
    AttnArgs af = a;
    if (!a.kn) {  // no new token: valid addresses for the kernel's unconditional loads (values unused)
      af.kn = af.vn = a.q;
      af.kn_sb = af.vn_sb = a.q_sb;
      af.kn_sh = af.vn_sh = 0;
    }
    const uint32_t groups = (uint32_t)kAttnBlock / (a.D / 4u), need = (a.nsplit + groups - 1u) / groups;
    const uint32_t n_new = nt ? 2u * (nt->nparts > 1u ? nt->nparts : 1u) : 0u;  // new-token workgroups: (K | V) x pieces
    // the ring kernel chose its split size from the device-side count, or a window moves the live count's start: the merge
    // instantiation that derives both from the count (with one-tile splits live_split_tokens is the host's TS)
    const bool rdev = a.t_dev && (a.stream_tpw || a.window > 0);
    const dim3 mgrid(a.Hq + n_new, a.B);
    if (kv_start) {  // a left-padded batch: the padded merges (per-row live splits), same shapes as below
      if (need <= 2u && (a.D == 128u || a.D == 64u) && a.nsplit <= 16u && tunables().attn_merge_wave != 0) {
        const dim3 wgrid((a.Hq + 3u) / 4u + n_new, a.B);
        KVQ_LAUNCH((decode_attn_merge_fast_padded_k<2>), wgrid, dim3(kAttnBlock), 0, st, af, nt ? *nt : none, (nt ? 1 : 0) | 2, a.kn ? 1 : 0);
      } else if (need <= 2u) KVQ_LAUNCH((decode_attn_merge_fast_padded_k<2>), mgrid, dim3(kAttnBlock), 0, st, af, nt ? *nt : none, nt ? 1 : 0, a.kn ? 1 : 0);
      else KVQ_LAUNCH((decode_attn_merge_fast_padded_k<kMergePF>), mgrid, dim3(kAttnBlock), 0, st, af, nt ? *nt : none, nt ? 1 : 0, a.kn ? 1 : 0);
    } else
    if (need <= 2u && (a.D == 128u || a.D == 64u) && a.nsplit <= 16u && tunables().attn_merge_wave != 0) {  // one wave per head, no workgroup
      const dim3 wgrid((a.Hq + 3u) / 4u + n_new, a.B);
      if (rdev) KVQ_LAUNCH((decode_attn_merge_fast_k<2, true>), wgrid, dim3(kAttnBlock), 0, st, af, nt ? *nt : none, (nt ? 1 : 0) | 2, a.kn ? 1 : 0);
      else KVQ_LAUNCH((decode_attn_merge_fast_k<2>), wgrid, dim3(kAttnBlock), 0, st, af, nt ? *nt : none, (nt ? 1 : 0) | 2, a.kn ? 1 : 0);
    } else if (need <= 2u && rdev) KVQ_LAUNCH((decode_attn_merge_fast_k<2, true>), mgrid, dim3(kAttnBlock), 0, st, af, nt ? *nt : none, nt ? 1 : 0, a.kn ? 1 : 0);
    else if (need <= 2u) KVQ_LAUNCH((decode_attn_merge_fast_k<2>), mgrid, dim3(kAttnBlock), 0, st, af, nt ? *nt : none, nt ? 1 : 0, a.kn ? 1 : 0);
    else if (rdev) KVQ_LAUNCH((decode_attn_merge_fast_k<kMergePF, true>), mgrid, dim3(kAttnBlock), 0, st, af, nt ? *nt : none, nt ? 1 : 0, a.kn ? 1 : 0);
    else KVQ_LAUNCH((decode_attn_merge_fast_k<kMergePF>), mgrid, dim3(kAttnBlock), 0, st, af, nt ? *nt : none, nt ? 1 : 0, a.kn ? 1 : 0);
  } else if (kv_start)
    KVQ_LAUNCH(decode_attn_merge_padded_k, dim3(a.Hq + (nt ? 2u * (nt->nparts > 1u ? nt->nparts : 1u) : 0u), a.B), dim3(kAttnBlock), 0, st, a, nt ? *nt : none,
                       nt ? 1 : 0);
  else
    KVQ_LAUNCH(decode_attn_merge_k, dim3(a.Hq + (nt ? 2u * (nt->nparts > 1u ? nt->nparts : 1u) : 0u), a.B), dim3(kAttnBlock), 0, st, a, nt ? *nt : none,
                       nt ? 1 : 0);
  return check_launch(name);
}

extern "C" {

// The split count is not monotone in T (tokens per split grow with T), so a decode loop that sizes
// its workspace ONCE for a capacity asks for the maximum over every T' <= T.
int64_t kvq_decode_attn_workspace_cap(const kvq_attn_dims_t* d) {
  if (!d || d->B <= 0 || d->Hq <= 0 || d->Hkv <= 0 || d->T < 0 || d->D <= 0) return -1;
  if (d->D != 32 && d->D != 64 && d->D != 128 && d->D != 256) return -1;
  kvq_attn_dims_t t = *d;
  uint32_t ts, ns, ns_max = 1;
  if (!plan(&t, &ts, &ns)) return -1;
  ns_max = ns > ns_max ? ns : ns_max;
  // kvq_decode_step_dev (device-side token count) always takes the one-tile plan, which can split finer than the
  // streaming plan a large batch gets: the capacity covers both
  if (plan_onetile(&t, &ts, &ns) && ns > ns_max) ns_max = ns;
  for (int64_t tt = 32; tt < d->T; tt += 32) {  // + 1 below covers a change of split size between two probes
    t.T = tt;
    if (plan(&t, &ts, &ns) && ns > ns_max) ns_max = ns;
    if (plan_onetile(&t, &ts, &ns) && ns > ns_max) ns_max = ns;
  }
  const int64_t rows = d->B * d->Hq * (int64_t)(ns_max + 1);
  const int64_t legacy = (rows * 2 + 3) / 4 * 4 + rows * d->D;
  return arrive_floats(d) + legacy;
}

int kvq_decode_attn(const void* q, int64_t q_sb, int64_t q_sh, const uint8_t* k_store, const kvq_strides_t* k_st,
                    const float* k_scales, int k_bits, const uint8_t* v_store, const kvq_strides_t* v_st,
                    const float* v_scales, int v_bits, const void* k_new, int64_t kn_sb, int64_t kn_sh,
                    const void* v_new, int64_t vn_sb, int64_t vn_sh, void* out, int64_t o_sb, int64_t o_sh, int dtype,
                    float sm_scale, float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* d,
                    void* stream) {
  return decode_attn_impl("kvq_decode_attn", q, q_sb, q_sh, k_store, k_st, k_scales, k_bits, v_store, v_st, v_scales, v_bits,
                          k_new, kn_sb, kn_sh, v_new, vn_sb, vn_sh, out, o_sb, o_sh, dtype, sm_scale, workspace,
                          workspace_floats, d, stream, nullptr);
}

}  // extern "C"

// Host-count decode under a sliding window of W keys: the query (at position T with a new token, T - 1 without) sees stored
// tokens [lo, T), lo = max(0, T + has_new - W). The store and its scales are viewed from row lo on and the call is planned for
// T - lo tokens: the kernels are the unwindowed ones over a shorter store, and rows before lo are never read.
static int64_t decode_window_lo(const kvq_attn_dims_t* d, const int64_t window, const bool has_new) {
  if (!d || window <= 0) return 0;
  const int64_t lo = d->T + (has_new ? 1 : 0) - window;
  return lo > 0 ? lo : 0;
}

extern "C" {

int kvq_decode_attn_window(const void* q, int64_t q_sb, int64_t q_sh, const uint8_t* k_store, const kvq_strides_t* k_st,
                           const float* k_scales, int k_bits, const uint8_t* v_store, const kvq_strides_t* v_st,
                           const float* v_scales, int v_bits, const void* k_new, int64_t kn_sb, int64_t kn_sh,
                           const void* v_new, int64_t vn_sb, int64_t vn_sh, void* out, int64_t o_sb, int64_t o_sh, int dtype,
                           float sm_scale, int64_t window, float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* d,
                           void* stream) {
  const char* name = "kvq_decode_attn_window";
  if (window < 0) {
    set_error("%s: window %lld must be >= 0 (0 = none)", name, (long long)window);
    return KVQ_E_DIMS;
  }
  const int64_t lo = decode_window_lo(d, window, k_new != nullptr);
  if (lo == 0)  // the window cuts nothing: today's call
    return decode_attn_impl(name, q, q_sb, q_sh, k_store, k_st, k_scales, k_bits, v_store, v_st, v_scales, v_bits, k_new, kn_sb,
                            kn_sh, v_new, vn_sb, vn_sh, out, o_sb, o_sh, dtype, sm_scale, workspace, workspace_floats, d, stream,
                            nullptr);
  if (!k_store || !v_store || !k_scales || !v_scales || !k_st || !v_st) {
    set_error("%s: NULL store / scales / strides", name);
    return KVQ_E_NULL;
  }
  kvq_attn_dims_t dw = *d;
  dw.T = d->T - lo;
  return decode_attn_impl(name, q, q_sb, q_sh, k_store + lo * k_st->t, k_st, k_scales + lo, k_bits, v_store + lo * v_st->t, v_st,
                          v_scales + lo, v_bits, k_new, kn_sb, kn_sh, v_new, vn_sb, vn_sh, out, o_sb, o_sh, dtype, sm_scale,
                          workspace, workspace_floats, &dw, stream, nullptr);
}

}  // extern "C"

extern "C" {

int kvq_decode_attn_padded(const void* q, int64_t q_sb, int64_t q_sh, const uint8_t* k_store, const kvq_strides_t* k_st,
                           const float* k_scales, int k_bits, const uint8_t* v_store, const kvq_strides_t* v_st,
                           const float* v_scales, int v_bits, const void* k_new, int64_t kn_sb, int64_t kn_sh,
                           const void* v_new, int64_t vn_sb, int64_t vn_sh, void* out, int64_t o_sb, int64_t o_sh, int dtype,
                           float sm_scale, int64_t window, const int32_t* kv_start, float* workspace, int64_t workspace_floats,
                           const kvq_attn_dims_t* d, void* stream) {
  if (!kv_start)  // exactly the windowed call
    return kvq_decode_attn_window(q, q_sb, q_sh, k_store, k_st, k_scales, k_bits, v_store, v_st, v_scales, v_bits, k_new, kn_sb,
                                  kn_sh, v_new, vn_sb, vn_sh, out, o_sb, o_sh, dtype, sm_scale, window, workspace, workspace_floats,
                                  d, stream);
  const char* name = "kvq_decode_attn_padded";
  if (window < 0) {
    set_error("%s: window %lld must be >= 0 (0 = none)", name, (long long)window);
    return KVQ_E_DIMS;
  }
  // per-row starts live on the device: no host-side lo, the store is passed whole and the padded kernels move each row's base
  return decode_attn_impl(name, q, q_sb, q_sh, k_store, k_st, k_scales, k_bits, v_store, v_st, v_scales, v_bits, k_new, kn_sb,
                          kn_sh, v_new, vn_sb, vn_sh, out, o_sb, o_sh, dtype, sm_scale, workspace, workspace_floats, d, stream,
                          nullptr, nullptr, window, kv_start);
}

}  // extern "C"

// Workgroups per new-token slice (NewTokenArgs::nparts): 1 up to the register path's 8,192 elements; past it one per 8,192
// elements when the slice takes 16-byte loads and aligned code stores (quant_new_token_parts), else 1 (the generic routine).
static uint32_t new_token_nparts(const NewTokenArgs& nt) {
  const int64_t n = (int64_t)nt.B * nt.H * nt.D;
  if (n <= 8192 || (nt.D != 128u && nt.D != 64u) || tunables().attn_new_token_parts == 0) return 1u;
  for (int w = 0; w < 2; ++w) {
    const int cb = nt.bits[w] == 8 ? 8 : 4;  // bytes of codes per 8-element vector
    if (!aligned(nt.x[w], 16) || (nt.xs_b[w] & 7) || (nt.xs_h[w] & 7) || !aligned(nt.q[w], (size_t)cb) || nt.qs_b[w] % cb || nt.qs_h[w] % cb || nt.qs_t[w] % cb) return 1u;
  }
  const int64_t parts = (n + 8191) / 8192;
  return (uint32_t)(parts > 32 ? 32 : parts);
}

// shared body of kvq_decode_step / kvq_decode_step_window (window 0: today's launches)
static int decode_step_impl(const char* name, const void* q, int64_t q_sb, int64_t q_sh, const void* k_new, int64_t kn_sb,
                            int64_t kn_sh, const void* v_new, int64_t vn_sb, int64_t vn_sh, uint8_t* k_store,
                            const kvq_strides_t* k_st, float* k_scales, int k_bits, uint8_t* v_store, const kvq_strides_t* v_st,
                            float* v_scales, int v_bits, void* out, int64_t o_sb, int64_t o_sh, int dtype, float sm_scale,
                            int64_t window, float eps, float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* d,
                            void* stream, const int32_t* kv_start = nullptr) {
  if (!d || !k_new || !v_new || !k_store || !v_store || !k_scales || !v_scales || !k_st || !v_st || !workspace) {
    set_error("%s: NULL argument", name);
    return KVQ_E_NULL;
  }
  if (window < 0) {
    set_error("%s: window %lld must be >= 0 (0 = none)", name, (long long)window);
    return KVQ_E_DIMS;
  }
  // a window: the attention reads the store from row lo on (decode_window_lo); the new token still goes into slot T
  // (a padded call has no host-side lo: the window rides in the launch beside kv_start, win_p)
  const int64_t lo = kv_start ? 0 : decode_window_lo(d, window, true);
  const int64_t win_p = kv_start ? window : 0;
  kvq_attn_dims_t dw = *d;
  dw.T = d->T - lo;
  const uint8_t* k_att = k_store + lo * k_st->t;
  const uint8_t* v_att = v_store + lo * v_st->t;
  const float* ks_att = k_scales + lo;
  const float* vs_att = v_scales + lo;
  // The new token's K / V go into slot T (append_from_past, ops.py:323-330). Small slices (the usual
  // case) are quantised by two extra workgroups of the attention's merge launch: a decode step is two
  // launches. Nothing reads slot T in that launch, and the partial kernel has read [0, T) before it.
  if (d->B * d->Hkv * d->D <= 65536 && (dtype == KVQ_F16 || dtype == KVQ_BF16) && d->T >= 0) {
    NewTokenArgs nt;
    nt.x[0] = k_new; nt.xs_b[0] = kn_sb; nt.xs_h[0] = kn_sh;
    nt.x[1] = v_new; nt.xs_b[1] = vn_sb; nt.xs_h[1] = vn_sh;
    nt.q[0] = k_store + d->T * k_st->t; nt.qs_b[0] = k_st->b; nt.qs_h[0] = k_st->h; nt.scale[0] = k_scales + d->T; nt.bits[0] = k_bits;
    nt.q[1] = v_store + d->T * v_st->t; nt.qs_b[1] = v_st->b; nt.qs_h[1] = v_st->h; nt.scale[1] = v_scales + d->T; nt.bits[1] = v_bits;
    nt.qs_t[0] = k_st->t; nt.qs_t[1] = v_st->t;
    nt.B = (uint32_t)d->B; nt.H = (uint32_t)d->Hkv; nt.D = (uint32_t)d->D; nt.eps = eps;
    nt.nparts = new_token_nparts(nt);
    return decode_attn_impl(name, q, q_sb, q_sh, k_att, k_st, ks_att, k_bits, v_att, v_st, vs_att, v_bits, k_new, kn_sb,
                            kn_sh, v_new, vn_sb, vn_sh, out, o_sb, o_sh, dtype, sm_scale, workspace, workspace_floats, &dw,
                            stream, &nt, nullptr, win_p, kv_start);
  }
  // large slices: attention first, then the regular quantise calls (stream order keeps the
  // attention's reads of [0, T) ahead of the writes to slot T)
  int rc = decode_attn_impl(name, q, q_sb, q_sh, k_att, k_st, ks_att, k_bits, v_att, v_st, vs_att, v_bits, k_new, kn_sb, kn_sh,
                            v_new, vn_sb, vn_sh, out, o_sb, o_sh, dtype, sm_scale, workspace, workspace_floats, &dw, stream, nullptr,
                            nullptr, win_p, kv_start);
  if (rc) return rc;
  const kvq_dims_t qd = {1, d->B, d->Hkv, 1, d->D};
  const kvq_strides_t kin = {0, kn_sb, kn_sh, d->D}, vin = {0, vn_sb, vn_sh, d->D};
  float* absmax_ws = workspace + arrive_floats(d);  // only the generic two-pass path uses it (1 float, behind the arrival words); the attention is already enqueued
  rc = k_bits == 8
           ? kvq_quant_i8_tokens(k_new, nullptr, &kin, dtype, reinterpret_cast<int8_t*>(k_store + d->T * k_st->t), k_st,
                                 k_scales + d->T, 0, absmax_ws, eps, &qd, stream)
           : kvq_quant_i4_tokens(k_new, nullptr, &kin, dtype, k_store + d->T * k_st->t, k_st, k_scales + d->T, 0,
                                 absmax_ws, eps, &qd, stream);
  if (rc) return rc;
  return v_bits == 8
             ? kvq_quant_i8_tokens(v_new, nullptr, &vin, dtype, reinterpret_cast<int8_t*>(v_store + d->T * v_st->t), v_st,
                                   v_scales + d->T, 0, absmax_ws, eps, &qd, stream)
             : kvq_quant_i4_tokens(v_new, nullptr, &vin, dtype, v_store + d->T * v_st->t, v_st, v_scales + d->T, 0,
                                   absmax_ws, eps, &qd, stream);
}

extern "C" {

int kvq_decode_step(const void* q, int64_t q_sb, int64_t q_sh, const void* k_new, int64_t kn_sb, int64_t kn_sh,
                    const void* v_new, int64_t vn_sb, int64_t vn_sh, uint8_t* k_store, const kvq_strides_t* k_st,
                    float* k_scales, int k_bits, uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales,
                    int v_bits, void* out, int64_t o_sb, int64_t o_sh, int dtype, float sm_scale, float eps,
                    float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* d, void* stream) {
  return decode_step_impl("kvq_decode_step", q, q_sb, q_sh, k_new, kn_sb, kn_sh, v_new, vn_sb, vn_sh, k_store, k_st, k_scales, k_bits,
                          v_store, v_st, v_scales, v_bits, out, o_sb, o_sh, dtype, sm_scale, 0, eps, workspace, workspace_floats, d,
                          stream);
}

int kvq_decode_step_window(const void* q, int64_t q_sb, int64_t q_sh, const void* k_new, int64_t kn_sb, int64_t kn_sh,
                           const void* v_new, int64_t vn_sb, int64_t vn_sh, uint8_t* k_store, const kvq_strides_t* k_st,
                           float* k_scales, int k_bits, uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales,
                           int v_bits, void* out, int64_t o_sb, int64_t o_sh, int dtype, float sm_scale, int64_t window, float eps,
                           float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* d, void* stream) {
  return decode_step_impl("kvq_decode_step_window", q, q_sb, q_sh, k_new, kn_sb, kn_sh, v_new, vn_sb, vn_sh, k_store, k_st, k_scales,
                          k_bits, v_store, v_st, v_scales, v_bits, out, o_sb, o_sh, dtype, sm_scale, window, eps, workspace,
                          workspace_floats, d, stream);
}

int kvq_decode_step_padded(const void* q, int64_t q_sb, int64_t q_sh, const void* k_new, int64_t kn_sb, int64_t kn_sh,
                           const void* v_new, int64_t vn_sb, int64_t vn_sh, uint8_t* k_store, const kvq_strides_t* k_st,
                           float* k_scales, int k_bits, uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales,
                           int v_bits, void* out, int64_t o_sb, int64_t o_sh, int dtype, float sm_scale, int64_t window,
                           const int32_t* kv_start, float eps, float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* d,
                           void* stream) {
  return decode_step_impl(kv_start ? "kvq_decode_step_padded" : "kvq_decode_step_window", q, q_sb, q_sh, k_new, kn_sb, kn_sh, v_new,
                          vn_sb, vn_sh, k_store, k_st, k_scales, k_bits, v_store, v_st, v_scales, v_bits, out, o_sb, o_sh, dtype,
                          sm_scale, window, eps, workspace, workspace_floats, d, stream, kv_start);
}

}  // extern "C"

// shared body of kvq_decode_step_dev / kvq_decode_step_dev_window: the window rides in the launch (AttnArgs::window)
static int decode_step_dev_impl(const char* name, const void* q, int64_t q_sb, int64_t q_sh, const void* k_new, int64_t kn_sb,
                                int64_t kn_sh, const void* v_new, int64_t vn_sb, int64_t vn_sh, uint8_t* k_store,
                                const kvq_strides_t* k_st, float* k_scales, int k_bits, uint8_t* v_store, const kvq_strides_t* v_st,
                                float* v_scales, int v_bits, void* out, int64_t o_sb, int64_t o_sh, int dtype, float sm_scale,
                                int64_t window, float eps, float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* d,
                                const int32_t* t_dev, void* stream, const int32_t* kv_start = nullptr) {
  if (window < 0) {
    set_error("%s: window %lld must be >= 0 (0 = none)", name, (long long)window);
    return KVQ_E_DIMS;
  }
  if (!d || !t_dev || !k_new || !v_new || !k_store || !v_store || !k_scales || !v_scales || !k_st || !v_st || !workspace) {
    set_error("%s: NULL argument", name);
    return KVQ_E_NULL;
  }
  if (d->T < 1 || d->B * d->Hkv * d->D > 65536 || (dtype != KVQ_F16 && dtype != KVQ_BF16)) {
    set_error("%s: needs an upper bound T >= 1, B * Hkv * D <= 65536 and fp16 / bf16 tensors", name);
    return KVQ_E_DIMS;
  }
  NewTokenArgs nt;  // slot 0: the merge launch adds the device-side T
  nt.x[0] = k_new; nt.xs_b[0] = kn_sb; nt.xs_h[0] = kn_sh;
  nt.x[1] = v_new; nt.xs_b[1] = vn_sb; nt.xs_h[1] = vn_sh;
  nt.q[0] = k_store; nt.qs_b[0] = k_st->b; nt.qs_h[0] = k_st->h; nt.qs_t[0] = k_st->t; nt.scale[0] = k_scales; nt.bits[0] = k_bits;
  nt.q[1] = v_store; nt.qs_b[1] = v_st->b; nt.qs_h[1] = v_st->h; nt.qs_t[1] = v_st->t; nt.scale[1] = v_scales; nt.bits[1] = v_bits;
  nt.B = (uint32_t)d->B; nt.H = (uint32_t)d->Hkv; nt.D = (uint32_t)d->D; nt.eps = eps;
  nt.nparts = new_token_nparts(nt);
  return decode_attn_impl(name, q, q_sb, q_sh, k_store, k_st, k_scales, k_bits, v_store, v_st, v_scales, v_bits, k_new, kn_sb,
                          kn_sh, v_new, vn_sb, vn_sh, out, o_sb, o_sh, dtype, sm_scale, workspace, workspace_floats, d,
                          stream, &nt, t_dev, window, kv_start);
}

extern "C" {

int kvq_decode_step_dev(const void* q, int64_t q_sb, int64_t q_sh, const void* k_new, int64_t kn_sb, int64_t kn_sh,
                        const void* v_new, int64_t vn_sb, int64_t vn_sh, uint8_t* k_store, const kvq_strides_t* k_st,
                        float* k_scales, int k_bits, uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales,
                        int v_bits, void* out, int64_t o_sb, int64_t o_sh, int dtype, float sm_scale, float eps,
                        float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* d, const int32_t* t_dev,
                        void* stream) {
  return decode_step_dev_impl("kvq_decode_step_dev", q, q_sb, q_sh, k_new, kn_sb, kn_sh, v_new, vn_sb, vn_sh, k_store, k_st, k_scales,
                              k_bits, v_store, v_st, v_scales, v_bits, out, o_sb, o_sh, dtype, sm_scale, 0, eps, workspace,
                              workspace_floats, d, t_dev, stream);
}

int kvq_decode_step_dev_window(const void* q, int64_t q_sb, int64_t q_sh, const void* k_new, int64_t kn_sb, int64_t kn_sh,
                               const void* v_new, int64_t vn_sb, int64_t vn_sh, uint8_t* k_store, const kvq_strides_t* k_st,
                               float* k_scales, int k_bits, uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales,
                               int v_bits, void* out, int64_t o_sb, int64_t o_sh, int dtype, float sm_scale, int64_t window,
                               float eps, float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* d,
                               const int32_t* t_dev, void* stream) {
  return decode_step_dev_impl("kvq_decode_step_dev_window", q, q_sb, q_sh, k_new, kn_sb, kn_sh, v_new, vn_sb, vn_sh, k_store, k_st,
                              k_scales, k_bits, v_store, v_st, v_scales, v_bits, out, o_sb, o_sh, dtype, sm_scale, window, eps,
                              workspace, workspace_floats, d, t_dev, stream);
}

int kvq_decode_step_dev_padded(const void* q, int64_t q_sb, int64_t q_sh, const void* k_new, int64_t kn_sb, int64_t kn_sh,
                               const void* v_new, int64_t vn_sb, int64_t vn_sh, uint8_t* k_store, const kvq_strides_t* k_st,
                               float* k_scales, int k_bits, uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales,
                               int v_bits, void* out, int64_t o_sb, int64_t o_sh, int dtype, float sm_scale, int64_t window,
                               const int32_t* kv_start, float eps, float* workspace, int64_t workspace_floats,
                               const kvq_attn_dims_t* d, const int32_t* t_dev, void* stream) {
  return decode_step_dev_impl(kv_start ? "kvq_decode_step_dev_padded" : "kvq_decode_step_dev_window", q, q_sb, q_sh, k_new, kn_sb,
                              kn_sh, v_new, vn_sb, vn_sh, k_store, k_st, k_scales, k_bits, v_store, v_st, v_scales, v_bits, out, o_sb,
                              o_sh, dtype, sm_scale, window, eps, workspace, workspace_floats, d, t_dev, stream, kv_start);
}

int kvq_decode_step_layers(int64_t n_layers, int append, const void* const* q, int64_t q_sb, int64_t q_sh,
                           const void* const* k_new, int64_t kn_sb, int64_t kn_sh, const void* const* v_new,
                           int64_t vn_sb, int64_t vn_sh, uint8_t* const* k_store, const kvq_strides_t* k_st,
                           float* const* k_scales, int k_bits, uint8_t* const* v_store, const kvq_strides_t* v_st,
                           float* const* v_scales, int v_bits, void* const* out, int64_t o_sb, int64_t o_sh, int dtype,
                           float sm_scale, float eps, float* workspace, int64_t workspace_floats,
                           const kvq_attn_dims_t* d, void* stream) {
  const char* name = "kvq_decode_step_layers";
  if (n_layers < 0 || !q || !out || !k_store || !v_store || !k_scales || !v_scales || (append && (!k_new || !v_new)) ||
      ((k_new == nullptr) != (v_new == nullptr))) {
    set_error("%s: NULL pointer table (or n_layers < 0)", name);
    return KVQ_E_NULL;
  }
  for (int64_t i = 0; i < n_layers; ++i) {
    const void* kn = k_new ? k_new[i] : nullptr;
    const void* vn = v_new ? v_new[i] : nullptr;
    const int rc = append ? kvq_decode_step(q[i], q_sb, q_sh, kn, kn_sb, kn_sh, vn, vn_sb, vn_sh, k_store[i], k_st, k_scales[i], k_bits,
                                            v_store[i], v_st, v_scales[i], v_bits, out[i], o_sb, o_sh, dtype, sm_scale, eps,
                                            workspace, workspace_floats, d, stream)
                          : kvq_decode_attn(q[i], q_sb, q_sh, k_store[i], k_st, k_scales[i], k_bits, v_store[i], v_st,
                                            v_scales[i], v_bits, kn, kn_sb, kn_sh, vn, vn_sb, vn_sh, out[i], o_sb, o_sh, dtype,
                                            sm_scale, workspace, workspace_floats, d, stream);
    if (rc) return rc;
  }
  return 0;
}

}  // extern "C"

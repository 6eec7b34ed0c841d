// host.inc — part of kvq_attn.hip (one translation unit, included in this order): the host side of decode attention.
//   plans          which kernel family serves the dims and how many splits (use_mfma, use_lds, plan, plan_onetile)
//   DecodeCall     one call as one record: every extern "C" entry point fills one and passes it on; the shared bodies
//                  (decode_attn_impl, decode_step_impl, decode_step_dev_impl) take the record, never the long lists
//   launch_partial the one selector of the partial launch: ring / one-tile MFMA / VALU, each in its plain, device-count (or
//                  windowed) or left-padded instantiation, picked as a host-stub pointer and launched once
//   launch_merge   the one selector of the merge launch: the fast family (by wave or per head) or the chained one
//   the extern "C" entry points, last
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
static bool use_lds(const kvq_attn_dims_t* d, int k_bits) {
  return tunables().attn_lds != 0 && use_mfma(d) && (d->D == 128 || (d->D == 64 && k_bits == 8));
}
constexpr int kStreamTC = 64;  // tokens per tile of the ring kernel
// ring kernel: tiles per wave (0 = one-tile splits). Chosen so that every wave of the launch is resident at once (one
// round) when the batch offers more 64-token tiles than the chip has wave slots.
static uint32_t stream_tpw(const kvq_attn_dims_t* d, int k_bits) {
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
// tpw_out (nullptr: not wanted): tiles per wave of the streaming layout when THAT is what the plan chose, 0 when it fell back
// to one-tile splits (the launcher must size its kernel choice from this, never from stream_tpw() on its own)
static bool plan(const kvq_attn_dims_t* d, uint32_t* ts, uint32_t* nsplit, uint32_t* tpw_out, int k_bits) {
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

// ---------------------------------------------------------------------------- workspace
// The workspace starts with one word per (batch row, kv head), padded to 16 bytes, in front of the partials: room for the
// arrival tickets of an in-launch merge that measured slower (r04b). Nothing uses them; the layout stays as it was.
static int64_t arrive_floats(const kvq_attn_dims_t* d) { return (d->B * d->Hkv + 3) / 4 * 4; }

static bool workspace_dims_ok(const kvq_attn_dims_t* d) {
  if (!d || d->B <= 0 || d->Hq <= 0 || d->Hkv <= 0 || d->T < 0 || d->D <= 0) return false;
  return d->D == 32 || d->D == 64 || d->D == 128 || d->D == 256;
}
// floats for nsplit splits: the arrival words, then (m, l) per (batch row, query head, split) padded to 16 bytes, then acc[D]
static int64_t workspace_floats_for(const kvq_attn_dims_t* d, const int64_t nsplit) {
  const int64_t rows = d->B * d->Hq * nsplit;
  return arrive_floats(d) + (rows * 2 + 3) / 4 * 4 + rows * d->D;
}
// kvq_decode_attn_workspace: what one call at exactly these dims needs, -1 for dims no plan serves
static int64_t decode_attn_workspace(const kvq_attn_dims_t* d) {
  if (!workspace_dims_ok(d)) return -1;
  uint32_t ts, ns, ns1;
  if (!plan(d, &ts, &ns, nullptr, 8)) return -1;
  // kvq_decode_step_dev always takes one-tile splits, which can be more than the streaming layout's: cover both
  if (plan_onetile(d, &ts, &ns1) && ns1 > ns) ns = ns1;
  return workspace_floats_for(d, ns > 0 ? ns : 1);
}

// ---------------------------------------------------------------------------- the call record
// One [B, H, D] tensor of a call (decode) or [B, H, S, D] (extend): base and element strides; decode leaves ss 0.
struct Rows {
  const void* p;
  int64_t sb, sh, ss;
};
struct OutRows {
  void* p;
  int64_t sb, sh, ss;
};
// One side (K or V) of the quantised store as the entry points take it: rows, byte strides, per-token scales, 8 or 4 bits.
struct StoreRef {
  const uint8_t* p;
  const kvq_strides_t* st;
  const float* scales;
  int bits;
};
// The store seen from stored row lo on (a sliding window's first visible row); s.st must not be NULL.
static StoreRef from_row(const StoreRef& s, const int64_t lo) { return StoreRef{s.p + lo * s.st->t, s.st, s.scales + lo, s.bits}; }
// The step entry points take their stores mutable (they write slot T); the record keeps the one const view the attention
// reads, and the two places that write slot T get the pointers back here.
static uint8_t* slot_rows(const StoreRef& s, const int64_t t) { return const_cast<uint8_t*>(s.p) + t * s.st->t; }
static float* slot_scale(const StoreRef& s, const int64_t t) { return const_cast<float*>(s.scales) + t; }

// One decode call, whichever entry point it came through. Fields an entry point does not have stay 0 / nullptr.
struct DecodeCall {
  const char* name;  // the entry point, for messages
  Rows q, k_new, v_new;
  OutRows out;
  StoreRef k, v;
  int dtype;
  float sm_scale, eps;
  float* workspace;
  int64_t workspace_floats;
  const kvq_attn_dims_t* d;
  void* stream;
  int64_t window;           // keys a query sees (0 = all)
  const int32_t* kv_start;  // device [B]: a left-padded batch
  const int32_t* t_dev;     // device word: the stored-token count of a graph-replayed step
  float softcap;            // the _ex entry points only: soft cap of the scores (0 = none)
  const float* sinks;       // the _ex entry points only: device [Hq] sink logits (NULL = none)
};
// The call seen from stored row lo: both stores and both scale tables shifted, T - lo tokens (*dims holds the new dims).
static DecodeCall from_row(const DecodeCall& c, const int64_t lo, kvq_attn_dims_t* dims) {
  DecodeCall w = c;
  *dims = *c.d;
  dims->T = c.d->T - lo;
  w.d = dims;
  w.k = from_row(c.k, lo);
  w.v = from_row(c.v, lo);
  return w;
}

// ---------------------------------------------------------------------------- checks decode and extend share
static int check_dtype(const char* name, const int dtype) {
  if (dtype == KVQ_F16 || dtype == KVQ_BF16) return 0;
  set_error("%s: dtype %d not supported (KVQ_F16, KVQ_BF16)", name, dtype);
  return KVQ_E_DTYPE;
}
static int check_bits(const char* name, const int k_bits, const int v_bits) {
  if ((k_bits == 8 || k_bits == 4) && (v_bits == 8 || v_bits == 4)) return 0;
  set_error("%s: k_bits / v_bits must be 8 or 4", name);
  return KVQ_E_DIMS;
}
static int check_store_rows(const char* name, const StoreRef& k, const StoreRef& v) {
  const int kal = k.bits == 8 ? 16 : 8, val = v.bits == 8 ? 16 : 8;
  if (aligned(k.p, kal) && k.st->b % kal == 0 && k.st->h % kal == 0 && k.st->t % kal == 0 && aligned(v.p, val) &&
      v.st->b % val == 0 && v.st->h % val == 0 && v.st->t % val == 0)
    return 0;
  set_error("%s: store rows must be %d / %d byte aligned", name, kal, val);
  return KVQ_E_DIMS;
}
// The score modifiers of an _ex call, checked, as the kernels' AttnMod. Both off: all zeros (mod_active false), and every
// selector below picks exactly what it picked before the modifiers existed.
static bool mod_active(const AttnMod& m) { return m.softcap > 0.0f || m.sinks != nullptr; }
static int attn_mod(const char* name, const float softcap, const float* sinks, AttnMod* out) {
  *out = AttnMod{0.0f, 0.0f, nullptr};
  if (!(softcap >= 0.0f) || softcap > FLT_MAX) {  // negative, NaN, inf
    set_error("%s: softcap %g must be a finite value >= 0 (0 = none)", name, (double)softcap);
    return KVQ_E_DIMS;
  }
  if (sinks) {
    if (const int rc = check_device(sinks, name)) return rc;
  }
  out->softcap = softcap;
  out->cap_k = softcap > 0.0f ? 2.88539008177792681f / softcap : 0.0f;  // 2 log2(e) / c
  out->sinks = sinks;
  return 0;
}
// A soft-capped call takes the capped partial kernels, which are built from the padded texts (kv_start NULL = every row starts at
// 0): like a padded call it has no host-side lo, the window rides in the launch and the padded merges count the live splits.
static bool padded_mode(const DecodeCall& c) { return c.kv_start != nullptr || c.softcap > 0.0f; }

// (k_bits, v_bits), each 8 or 4, as compile-time constants: f(std::integral_constant<int, KBITS>, <int, VBITS>)
template <class F>
static void with_bits(const int k_bits, const int v_bits, F&& f) {
  typedef std::integral_constant<int, 8> I8;
  typedef std::integral_constant<int, 4> I4;
  if (k_bits == 8 && v_bits == 8) f(I8{}, I8{});
  else if (k_bits == 8) f(I8{}, I4{});
  else if (v_bits == 8) f(I4{}, I8{});
  else f(I4{}, I4{});
}

// ---------------------------------------------------------------------------- the partial launch
// Which instantiation of a kernel family serves the call. kCount: the count is a device word — every ring launch of such a
// call (TDEV), and the one-tile / VALU kernels only under a window (*_window_k: the host-count ones never evaluate it).
enum PartialVariant { kPlain, kCount, kPadded };
typedef void (*RingKernel)(const AttnArgs, const uint32_t);
typedef void (*TileKernel)(const AttnArgs);

template <int KBITS, int VBITS, int TG, int HD>
static RingKernel ring_kernel(const PartialVariant v) {
  if (v == kPadded) return decode_attn_lds_mfma_padded_k<KBITS, VBITS, 64, KBITS == 8, 2, TG, HD>;
  if (v == kCount) return decode_attn_lds_mfma_k<KBITS, VBITS, 64, KBITS == 8, 2, TG, HD, true>;
  return decode_attn_lds_mfma_k<KBITS, VBITS, 64, KBITS == 8, 2, TG, HD>;
}
template <int KBITS, int VBITS, int HD>
static TileKernel tile_kernel(const PartialVariant v) {
  if (v == kPadded) return decode_attn_partial_mfma_padded_k<KBITS, VBITS, kAttnMfmaTC, HD>;
  if (v == kCount) return decode_attn_partial_mfma_window_k<KBITS, VBITS, kAttnMfmaTC, HD>;
  return decode_attn_partial_mfma_k<KBITS, VBITS, kAttnMfmaTC, HD>;
}
template <int KBITS, int VBITS, int NQ>
static TileKernel valu_kernel(const PartialVariant v) {
  if (v == kPadded) return decode_attn_partial_padded_k<KBITS, VBITS, NQ>;
  if (v == kCount) return decode_attn_partial_window_k<KBITS, VBITS, NQ>;
  return decode_attn_partial_k<KBITS, VBITS, NQ>;
}

// The one selector of the partial launch, for a host count, a device count and a left-padded batch alike: the route (ring at
// head_dim 64 / 128, one-tile MFMA, VALU by query heads per kv head) is decided once, the variant picks the instantiation.
// The soft-capped instantiations (decode_attn_*_mod_k): one per family, whatever the count, window and starts.
typedef void (*RingModKernel)(const AttnArgs, const uint32_t, const AttnMod);
typedef void (*TileModKernel)(const AttnArgs, const AttnMod);
template <int KBITS, int VBITS, int TG, int HD>
static RingModKernel ring_mod_kernel() { return decode_attn_lds_mfma_mod_k<KBITS, VBITS, 64, KBITS == 8, 2, TG, HD>; }

template <int KBITS, int VBITS>
static void launch_partial(const AttnArgs& a, const AttnMod& mod, hipStream_t st) {
  const dim3 grid(a.nsplit, a.Hkv, a.B);
  // INT8 keys in the streaming kernel: the stored bytes straight into the int8 MFMA, the query as two int8 planes whose cost
  // is amortised over the wave's tiles (50.6 vs 52.3 us per call at batch 8). head_dim 64 rides the ring with INT8 keys only.
  constexpr bool kI8 = KBITS == 8;
  const bool ring = a.mfma && a.stream_tpw && a.lds && (a.D == 128u || (kI8 && a.D == 64u));
  const bool count = a.t_dev && (ring || a.window > 0);
  const PartialVariant v = a.kv_start ? kPadded : count ? kCount : kPlain;
  if (mod.softcap > 0.0f) {  // the same route, the capped instantiation (sinks alone change only the merge)
    if (ring) {
      const size_t slot = 64 * (a.D * KBITS / 8 + a.D * VBITS / 8) + 512;
      RingModKernel k = ring_mod_kernel<KBITS, VBITS, 1, 128>();
      if constexpr (kI8) {
        const bool tg4 = a.nq <= 4u;
        if (a.D == 64u) k = tg4 ? ring_mod_kernel<KBITS, VBITS, 4, 64>() : ring_mod_kernel<KBITS, VBITS, 1, 64>();
        else if (tg4) k = ring_mod_kernel<KBITS, VBITS, 4, 128>();
      }
      launch(k, grid, dim3(kWave), 2 * slot, st, a, a.stream_tpw, mod);
      return;
    }
    TileModKernel k;
    if (a.mfma) k = a.D == 64u ? decode_attn_partial_mfma_mod_k<KBITS, VBITS, kAttnMfmaTC, 64> : decode_attn_partial_mfma_mod_k<KBITS, VBITS, kAttnMfmaTC, 128>;
    else if (a.nq == 1) k = decode_attn_partial_mod_k<KBITS, VBITS, 1>;
    else if (a.nq == 2) k = decode_attn_partial_mod_k<KBITS, VBITS, 2>;
    else if (a.nq <= 4) k = decode_attn_partial_mod_k<KBITS, VBITS, 4>;
    else k = decode_attn_partial_mod_k<KBITS, VBITS, 8>;
    launch(k, grid, dim3(a.mfma ? kWave : kAttnBlock), 0, st, a, mod);
    return;
  }
  if (ring) {
    // ring depth 2: one tile in flight behind the one being reduced, four one-wave workgroups per CU (25.6 KiB each for
    // INT8 keys + INT4 values; eight per CU at head_dim 64). Measured at batch 8, 16 K tokens (per layer call incl. merge,
    // profiles/r03d_*): depth 2 40.8 us, depth 3 44.7 us, depth 4 (three workgroups per CU) 86 us; 32-token tiles 42.1-51.6 us.
    const size_t slot = 64 * (a.D * KBITS / 8 + a.D * VBITS / 8) + 512;
    RingKernel k = ring_kernel<KBITS, VBITS, 1, 128>(v);
    if constexpr (kI8) {  // at most 4 query heads per kv head: one score output per tile (AttnStream TG = 4)
      const bool tg4 = a.nq <= 4u;
      if (a.D == 64u) k = tg4 ? ring_kernel<KBITS, VBITS, 4, 64>(v) : ring_kernel<KBITS, VBITS, 1, 64>(v);
      else if (tg4) k = ring_kernel<KBITS, VBITS, 4, 128>(v);
    }
    launch(k, grid, dim3(kWave), 2 * slot, st, a, a.stream_tpw);
    return;
  }
  TileKernel k;
  if (a.mfma) k = a.D == 64u ? tile_kernel<KBITS, VBITS, 64>(v) : tile_kernel<KBITS, VBITS, 128>(v);
  else if (a.nq == 1) k = valu_kernel<KBITS, VBITS, 1>(v);
  else if (a.nq == 2) k = valu_kernel<KBITS, VBITS, 2>(v);
  else if (a.nq <= 4) k = valu_kernel<KBITS, VBITS, 4>(v);
  else k = valu_kernel<KBITS, VBITS, 8>(v);
  launch(k, grid, dim3(a.mfma ? kWave : kAttnBlock), 0, st, a);
}

// ---------------------------------------------------------------------------- the merge launch
typedef void (*MergeFastKernel)(const AttnArgs, const NewTokenArgs, const int, const int);
typedef void (*MergeChainedKernel)(const AttnArgs, const NewTokenArgs, const int);

// The one selector of the merge launch. nt != nullptr: the launch also quantises the new token into its slot, with
// 2 * max(nparts, 1) extra workgroups ((K | V) x pieces).
typedef void (*MergeFastModKernel)(const AttnArgs, const NewTokenArgs, const int, const int, const AttnMod);
typedef void (*MergeChainedModKernel)(const AttnArgs, const NewTokenArgs, const int, const AttnMod);
// mod active (a soft cap or sinks): the same selection among the *_mod_k forms; `padded` then also covers a soft-capped call
// without per-row starts (padded_mode).
static void launch_merge(const AttnArgs& a, const NewTokenArgs* nt, const AttnMod& mod, const bool padded, hipStream_t st) {
  const NewTokenArgs nta = nt ? *nt : NewTokenArgs{};
  const uint32_t n_new = nt ? 2u * (nt->nparts > 1u ? nt->nparts : 1u) : 0u;
  const int fuse = nt ? 1 : 0, has_new = a.kn ? 1 : 0;
  const bool modk = mod_active(mod);
  if (!(a.nsplit >= 1u && a.nsplit <= (uint32_t)kAttnBlock && a.D <= (uint32_t)kAttnBlock && tunables().attn_merge_fast)) {
    if (modk) {
      const MergeChainedModKernel k = padded ? decode_attn_merge_padded_mod_k : decode_attn_merge_mod_k;
      launch(k, dim3(a.Hq + n_new, a.B), dim3(kAttnBlock), 0, st, a, nta, fuse, mod);
      return;
    }
    const MergeChainedKernel k = padded ? decode_attn_merge_padded_k : decode_attn_merge_k;
    launch(k, dim3(a.Hq + n_new, a.B), dim3(kAttnBlock), 0, st, a, nta, fuse);
    return;
  }
  AttnArgs af = a;
  if (!a.kn) {  // no new token: valid addresses for the kernel's unconditional loads (values unused)
    af.kn = af.vn = a.q;
    af.kn_sb = af.vn_sb = a.q_sb;
    af.kn_sh = af.vn_sh = 0;
  }
  const uint32_t groups = (uint32_t)kAttnBlock / (a.D / 4u), need = (a.nsplit + groups - 1u) / groups;
  // the ring kernel chose its split size from the device-side count, or a window moves the live count's start: the merge
  // instantiation that derives both from the count (with one-tile splits live_split_tokens is the host's TS)
  const bool rdev = a.t_dev && (a.stream_tpw || a.window > 0);
  // one wave per head, no workgroup (four heads per workgroup of the grid)
  const bool by_wave = need <= 2u && (a.D == 128u || a.D == 64u) && a.nsplit <= 16u && tunables().attn_merge_wave != 0;
  const dim3 mgrid((by_wave ? (a.Hq + 3u) / 4u : a.Hq) + n_new, a.B);
  if (modk) {
    MergeFastModKernel k;
    if (padded) k = need <= 2u ? decode_attn_merge_fast_padded_mod_k<2> : decode_attn_merge_fast_padded_mod_k<kMergePF>;
    else if (need <= 2u) k = rdev ? decode_attn_merge_fast_mod_k<2, true> : decode_attn_merge_fast_mod_k<2>;
    else k = rdev ? decode_attn_merge_fast_mod_k<kMergePF, true> : decode_attn_merge_fast_mod_k<kMergePF>;
    launch(k, mgrid, dim3(kAttnBlock), 0, st, af, nta, fuse | (by_wave ? 2 : 0), has_new, mod);
    return;
  }
  MergeFastKernel k;
  if (padded) k = need <= 2u ? decode_attn_merge_fast_padded_k<2> : decode_attn_merge_fast_padded_k<kMergePF>;
  else if (need <= 2u) k = rdev ? decode_attn_merge_fast_k<2, true> : decode_attn_merge_fast_k<2>;
  else k = rdev ? decode_attn_merge_fast_k<kMergePF, true> : decode_attn_merge_fast_k<kMergePF>;
  launch(k, mgrid, dim3(kAttnBlock), 0, st, af, nta, fuse | (by_wave ? 2 : 0), has_new);
}

// ---------------------------------------------------------------------------- the shared bodies
// every decode entry point ends here; nt != nullptr: quantise the new token in the merge launch
static int decode_attn_impl(const DecodeCall& c, const NewTokenArgs* nt) {
  const char* name = c.name;
  const kvq_attn_dims_t* d = c.d;
  const int32_t* t_dev = c.t_dev;
  if (!d || !c.q.p || !c.out.p) {
    set_error("%s: NULL q / out / dims", name);
    return KVQ_E_NULL;
  }
  if (const int rcd = check_device(c.out.p, name)) return rcd;
  if (c.kv_start) {
    if (const int rcd = check_device(c.kv_start, name)) return rcd;
  }
  AttnMod mod;
  if (const int rc = attn_mod(name, c.softcap, c.sinks, &mod)) return rc;
  const bool padded = padded_mode(c);  // a.kv_start may still be NULL: the capped kernels and the *_padded_mod_k merges read that as 0
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
  if (const int rc = check_dtype(name, c.dtype)) return rc;
  if (const int rc = check_bits(name, c.k.bits, c.v.bits)) return rc;
  if ((c.k_new.p == nullptr) != (c.v_new.p == nullptr)) {
    set_error("%s: k_new and v_new must be given together", name);
    return KVQ_E_NULL;
  }
  const bool has_new = c.k_new.p != nullptr;
  if (d->T == 0 && !has_new) {
    set_error("%s: nothing to attend to (T == 0 and no new token)", name);
    return KVQ_E_DIMS;
  }
  if (d->T > 0 && (!c.k.p || !c.v.p || !c.k.scales || !c.v.scales || !c.k.st || !c.v.st || !c.workspace)) {
    set_error("%s: NULL store / scales / strides / workspace", name);
    return KVQ_E_NULL;
  }
  // A device-side count under a window attends at most W - 1 stored tokens whatever the count: the grid and the split layout
  // are planned for that (pd), while a.T stays the caller's bound (the clamp of the count and of the new-token slot).
  kvq_attn_dims_t dp = *d;
  if (t_dev && c.window > 0 && c.window - 1 < d->T) dp.T = c.window - 1;
  // A padded call, host count or device count: per-row starts live on the device, so the grid is planned for what the window
  // alone leaves visible (W keys with the query's own: W - 1 stored ones beside a new token, W without one)
  if (padded && c.window > 0 && c.window - (has_new ? 1 : 0) < d->T) dp.T = c.window - (has_new ? 1 : 0);
  const kvq_attn_dims_t* pd = &dp;
  const int64_t need = decode_attn_workspace(pd);
  if (d->T > 0 && c.workspace_floats < need) {
    set_error("%s: workspace of %lld floats, %lld needed", name, (long long)c.workspace_floats, (long long)need);
    return KVQ_E_DIMS;
  }
  if (d->T > 0) {
    if (const int rc = check_store_rows(name, c.k, c.v)) return rc;
  }
  if (d->T > 0 && (d->T * c.k.st->t >= (int64_t(1) << 31) || d->T * c.v.st->t >= (int64_t(1) << 31))) {
    set_error("%s: one (batch, kv head) row of the store must stay below 2 GiB", name);
    return KVQ_E_DIMS;
  }
  if (!aligned(c.q.p, 16) || c.q.sb % 8 || c.q.sh % 8) {
    set_error("%s: q must be 16-byte aligned with strides that are multiples of 8 elements", name);
    return KVQ_E_DIMS;
  }
  AttnArgs a;
  a.q = c.q.p; a.q_sb = c.q.sb; a.q_sh = c.q.sh;
  a.k = c.k.p; a.v = c.v.p;
  if (d->T > 0) {
    a.k_sb = c.k.st->b; a.k_sh = c.k.st->h; a.k_st = c.k.st->t;
    a.v_sb = c.v.st->b; a.v_sh = c.v.st->h; a.v_st = c.v.st->t;
  } else {
    a.k_sb = a.k_sh = a.k_st = a.v_sb = a.v_sh = a.v_st = 0;
  }
  a.k_scale = c.k.scales; a.v_scale = c.v.scales;
  a.kn = c.k_new.p; a.kn_sb = c.k_new.sb; a.kn_sh = c.k_new.sh;
  a.vn = c.v_new.p; a.vn_sb = c.v_new.sb; a.vn_sh = c.v_new.sh;
  a.out = c.out.p; a.o_sb = c.out.sb; a.o_sh = c.out.sh;
  const int64_t arrive_n = arrive_floats(d);
  a.ws = c.workspace ? c.workspace + arrive_n : c.workspace;
  const int64_t ws_floats = c.workspace_floats - arrive_n;
  a.kv_start = c.kv_start;  // read by the *_padded_k kernels only
  a.ws_bytes = 0u;
  a.window = (t_dev || padded) ? (int32_t)(c.window < INT32_MAX ? c.window : INT32_MAX) : 0;
  a.sm_scale = c.sm_scale;
  a.B = (uint32_t)d->B; a.Hq = (uint32_t)d->Hq; a.Hkv = (uint32_t)d->Hkv; a.T = (uint32_t)d->T; a.D = (uint32_t)d->D;
  a.nq = (uint32_t)(d->Hq / d->Hkv);
  a.lpt_shift = ilog2_exact(d->D / 16);
  a.dtype = c.dtype;
  a.mfma = use_mfma(d) ? 1 : 0;
  a.stream_tpw = 0u;
  // a device-side count (graph replay) takes the ring kernel too — its waves spread the live tiles over the launch (ring_dev_tpw) —
  // unless the knob says one-tile splits as before (attn_ring_dev = 0)
  const bool ring_dev = t_dev && tunables().attn_ring_dev != 0;
  a.lds = ((!t_dev || ring_dev) && use_lds(pd, c.k.bits)) ? 1u : 0u;
  a.t_dev = t_dev;
  if (!((t_dev && !ring_dev) ? plan_onetile(pd, &a.TS, &a.nsplit) : plan(pd, &a.TS, &a.nsplit, &a.stream_tpw, c.k.bits))) {
    set_error("%s: T=%lld needs more than %d splits of %d tokens", name, (long long)d->T, kAttnMaxSplit, kAttnMaxTS);
    return KVQ_E_DIMS;
  }
  a.acc_off = ((int64_t)a.B * a.Hq * a.nsplit * 2 + 3) / 4 * 4;
  // the split layout actually chosen (a device-side T always takes one-tile splits) must fit too
  if (d->T > 0 && ws_floats < a.acc_off + (int64_t)a.B * a.Hq * a.nsplit * a.D) {
    set_error("%s: workspace of %lld floats, %lld needed for %u splits", name, (long long)ws_floats,
              (long long)(a.acc_off + (int64_t)a.B * a.Hq * a.nsplit * a.D), a.nsplit);
    return KVQ_E_DIMS;
  }
  if (d->T > 0 && !aligned(c.workspace, 16)) {
    set_error("%s: workspace must be 16-byte aligned", name);
    return KVQ_E_DIMS;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
  if (a.nsplit > 0) {
    with_bits(c.k.bits, c.v.bits, [&](auto kb, auto vb) { launch_partial<decltype(kb)::value, decltype(vb)::value>(a, mod, st); });
    if (const int rc = check_launch(name)) return rc;
  }
  launch_merge(a, nt, mod, padded, st);
  return check_launch(name);
}

// Host-count decode under a sliding window of W keys: the query (at position T with a new token, T - 1 without) sees stored
// tokens [lo, T), lo = max(0, T + has_new - W). The call is seen from row lo on (from_row) and planned for T - lo tokens: the
// kernels are the unwindowed ones over a shorter store, and rows before lo are never read.
static int64_t decode_window_lo(const kvq_attn_dims_t* d, const int64_t window, const bool has_new) {
  if (!d || window <= 0) return 0;
  const int64_t lo = d->T + (has_new ? 1 : 0) - window;
  return lo > 0 ? lo : 0;
}
static int check_window(const DecodeCall& c) {
  if (c.window >= 0) return 0;
  set_error("%s: window %lld must be >= 0 (0 = none)", c.name, (long long)c.window);
  return KVQ_E_DIMS;
}

// kvq_decode_attn_window (and _padded without kv_start)
static int decode_attn_window_impl(const DecodeCall& c) {
  if (const int rc = check_window(c)) return rc;
  const int64_t lo = decode_window_lo(c.d, c.window, c.k_new.p != nullptr);
  DecodeCall w = c;
  w.window = 0;  // applied here, on the host
  if (lo == 0) return decode_attn_impl(w, nullptr);  // the window cuts nothing: the unwindowed call
  if (!c.k.p || !c.v.p || !c.k.scales || !c.v.scales || !c.k.st || !c.v.st) {
    set_error("%s: NULL store / scales / strides", c.name);
    return KVQ_E_NULL;
  }
  kvq_attn_dims_t dw;
  return decode_attn_impl(from_row(w, lo, &dw), nullptr);
}

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
// The new token of a step call, quantised into stored row `slot` (a host count: T; a device count: 0, the merge launch adds
// the device word), nparts included. The call's new-token tensors, stores and strides must not be NULL.
static NewTokenArgs new_token_args(const DecodeCall& c, const int64_t slot) {
  NewTokenArgs nt;
  const Rows* x[2] = {&c.k_new, &c.v_new};
  const StoreRef* s[2] = {&c.k, &c.v};
  for (int w = 0; w < 2; ++w) {
    nt.x[w] = x[w]->p; nt.xs_b[w] = x[w]->sb; nt.xs_h[w] = x[w]->sh;
    nt.q[w] = slot_rows(*s[w], slot); nt.qs_b[w] = s[w]->st->b; nt.qs_h[w] = s[w]->st->h; nt.qs_t[w] = s[w]->st->t;
    nt.scale[w] = slot_scale(*s[w], slot); nt.bits[w] = s[w]->bits;
  }
  nt.B = (uint32_t)c.d->B; nt.H = (uint32_t)c.d->Hkv; nt.D = (uint32_t)c.d->D; nt.eps = c.eps;
  nt.nparts = new_token_nparts(nt);
  return nt;
}

// kvq_decode_step / _window / _padded (window 0 and no kv_start: the plain step's launches)
static int decode_step_impl(const DecodeCall& c) {
  const kvq_attn_dims_t* d = c.d;
  if (!d || !c.k_new.p || !c.v_new.p || !c.k.p || !c.v.p || !c.k.scales || !c.v.scales || !c.k.st || !c.v.st || !c.workspace) {
    set_error("%s: NULL argument", c.name);
    return KVQ_E_NULL;
  }
  if (const int rc = check_window(c)) return rc;
  // a window: the attention reads the store from row lo on (decode_window_lo); the new token still goes into slot T
  // (a padded call has no host-side lo: the window rides in the launch beside kv_start)
  kvq_attn_dims_t dw;
  DecodeCall att = from_row(c, padded_mode(c) ? 0 : decode_window_lo(d, c.window, true), &dw);
  if (!padded_mode(c)) att.window = 0;
  // The new token's K / V go into slot T (append_from_past, ops.py:323-330). Small slices (the usual
  // case) are quantised by two extra workgroups of the attention's merge launch: a decode step is two
  // launches. Nothing reads slot T in that launch, and the partial kernel has read [0, T) before it.
  if (d->B * d->Hkv * d->D <= 65536 && (c.dtype == KVQ_F16 || c.dtype == KVQ_BF16) && d->T >= 0) {
    const NewTokenArgs nt = new_token_args(c, d->T);
    return decode_attn_impl(att, &nt);
  }
  // large slices: attention first, then the regular quantise calls (stream order keeps the
  // attention's reads of [0, T) ahead of the writes to slot T)
  if (const int rc = decode_attn_impl(att, nullptr)) return rc;
  const kvq_dims_t qd = {1, d->B, d->Hkv, 1, d->D};
  float* absmax_ws = c.workspace + arrive_floats(d);  // only the generic two-pass path uses it (1 float, behind the arrival words); the attention is already enqueued
  const Rows* x[2] = {&c.k_new, &c.v_new};
  const StoreRef* s[2] = {&c.k, &c.v};
  for (int w = 0; w < 2; ++w) {
    const kvq_strides_t in = {0, x[w]->sb, x[w]->sh, d->D};
    uint8_t* rows = slot_rows(*s[w], d->T);
    const int rc = s[w]->bits == 8 ? kvq_quant_i8_tokens(x[w]->p, nullptr, &in, c.dtype, reinterpret_cast<int8_t*>(rows), s[w]->st,
                                                         slot_scale(*s[w], d->T), 0, absmax_ws, c.eps, &qd, c.stream)
                                   : kvq_quant_i4_tokens(x[w]->p, nullptr, &in, c.dtype, rows, s[w]->st, slot_scale(*s[w], d->T), 0,
                                                         absmax_ws, c.eps, &qd, c.stream);
    if (rc) return rc;
  }
  return 0;
}

// kvq_decode_step_dev / _window / _padded: the window rides in the launch (AttnArgs::window)
static int decode_step_dev_impl(const DecodeCall& c) {
  const kvq_attn_dims_t* d = c.d;
  if (const int rc = check_window(c)) return rc;
  if (!d || !c.t_dev || !c.k_new.p || !c.v_new.p || !c.k.p || !c.v.p || !c.k.scales || !c.v.scales || !c.k.st || !c.v.st || !c.workspace) {
    set_error("%s: NULL argument", c.name);
    return KVQ_E_NULL;
  }
  if (d->T < 1 || d->B * d->Hkv * d->D > 65536 || (c.dtype != KVQ_F16 && c.dtype != KVQ_BF16)) {
    set_error("%s: needs an upper bound T >= 1, B * Hkv * D <= 65536 and fp16 / bf16 tensors", c.name);
    return KVQ_E_DIMS;
  }
  const NewTokenArgs nt = new_token_args(c, 0);  // slot 0: the merge launch adds the device-side T
  return decode_attn_impl(c, &nt);
}

}  // namespace kvq

using namespace kvq;

// Every entry point fills one DecodeCall from its argument list, field by name, and passes it on: the only place the long
// lists exist. The thirteen entry points name their shared parameters alike (include/kvq_hip.h), so the shared fields are filled by
// one text; window, kv_start, eps and t_dev are set by the entry points that have them.
#define KVQ_DECODE_CALL(NAME)                                                                                                \
  DecodeCall c = {};                                                                                                         \
  c.name = NAME;                                                                                                             \
  c.q = {q, q_sb, q_sh, 0}; c.k_new = {k_new, kn_sb, kn_sh, 0}; c.v_new = {v_new, vn_sb, vn_sh, 0}; c.out = {out, o_sb, o_sh, 0}; \
  c.k = {k_store, k_st, k_scales, k_bits}; c.v = {v_store, v_st, v_scales, v_bits};                                          \
  c.dtype = dtype; c.sm_scale = sm_scale; c.workspace = workspace; c.workspace_floats = workspace_floats; c.d = d; c.stream = stream

extern "C" {

int64_t kvq_decode_attn_workspace(const kvq_attn_dims_t* d) { return decode_attn_workspace(d); }

// The split count is not monotone in T (tokens per split grow with T), so a decode loop that sizes
// its workspace ONCE for a capacity asks for the maximum over every T' <= T.
int64_t kvq_decode_attn_workspace_cap(const kvq_attn_dims_t* d) {
  if (!workspace_dims_ok(d)) return -1;
  kvq_attn_dims_t t = *d;
  uint32_t ts, ns, ns_max = 1;
  if (!plan(&t, &ts, &ns, nullptr, 8)) return -1;
  ns_max = ns > ns_max ? ns : ns_max;
  // kvq_decode_step_dev (device-side token count) always takes the one-tile plan, which can split finer than the
  // streaming plan a large batch gets: the capacity covers both
  if (plan_onetile(&t, &ts, &ns) && ns > ns_max) ns_max = ns;
  for (int64_t tt = 32; tt < d->T; tt += 32) {  // + 1 below covers a change of split size between two probes
    t.T = tt;
    if (plan(&t, &ts, &ns, nullptr, 8) && ns > ns_max) ns_max = ns;
    if (plan_onetile(&t, &ts, &ns) && ns > ns_max) ns_max = ns;
  }
  return workspace_floats_for(d, (int64_t)ns_max + 1);
}

int kvq_decode_attn(const void* q, int64_t q_sb, int64_t q_sh, const uint8_t* k_store, const kvq_strides_t* k_st,
                    const float* k_scales, int k_bits, const uint8_t* v_store, const kvq_strides_t* v_st,
                    const float* v_scales, int v_bits, const void* k_new, int64_t kn_sb, int64_t kn_sh,
                    const void* v_new, int64_t vn_sb, int64_t vn_sh, void* out, int64_t o_sb, int64_t o_sh, int dtype,
                    float sm_scale, float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* d,
                    void* stream) {
  KVQ_DECODE_CALL("kvq_decode_attn");
  return decode_attn_impl(c, nullptr);
}

int kvq_decode_attn_window(const void* q, int64_t q_sb, int64_t q_sh, const uint8_t* k_store, const kvq_strides_t* k_st,
                           const float* k_scales, int k_bits, const uint8_t* v_store, const kvq_strides_t* v_st,
                           const float* v_scales, int v_bits, const void* k_new, int64_t kn_sb, int64_t kn_sh,
                           const void* v_new, int64_t vn_sb, int64_t vn_sh, void* out, int64_t o_sb, int64_t o_sh, int dtype,
                           float sm_scale, int64_t window, float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* d,
                           void* stream) {
  KVQ_DECODE_CALL("kvq_decode_attn_window");
  c.window = window;
  return decode_attn_window_impl(c);
}

int kvq_decode_attn_padded(const void* q, int64_t q_sb, int64_t q_sh, const uint8_t* k_store, const kvq_strides_t* k_st,
                           const float* k_scales, int k_bits, const uint8_t* v_store, const kvq_strides_t* v_st,
                           const float* v_scales, int v_bits, const void* k_new, int64_t kn_sb, int64_t kn_sh,
                           const void* v_new, int64_t vn_sb, int64_t vn_sh, void* out, int64_t o_sb, int64_t o_sh, int dtype,
                           float sm_scale, int64_t window, const int32_t* kv_start, float* workspace, int64_t workspace_floats,
                           const kvq_attn_dims_t* d, void* stream) {
  KVQ_DECODE_CALL(kv_start ? "kvq_decode_attn_padded" : "kvq_decode_attn_window");
  c.window = window;
  c.kv_start = kv_start;
  if (!kv_start) return decode_attn_window_impl(c);  // exactly the windowed call
  if (const int rc = check_window(c)) return rc;
  // per-row starts live on the device: no host-side lo, the store is passed whole and the padded kernels move each row's base
  return decode_attn_impl(c, nullptr);
}

int kvq_decode_step(const void* q, int64_t q_sb, int64_t q_sh, const void* k_new, int64_t kn_sb, int64_t kn_sh,
                    const void* v_new, int64_t vn_sb, int64_t vn_sh, uint8_t* k_store, const kvq_strides_t* k_st,
                    float* k_scales, int k_bits, uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales,
                    int v_bits, void* out, int64_t o_sb, int64_t o_sh, int dtype, float sm_scale, float eps,
                    float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* d, void* stream) {
  KVQ_DECODE_CALL("kvq_decode_step");
  c.eps = eps;
  return decode_step_impl(c);
}

int kvq_decode_step_window(const void* q, int64_t q_sb, int64_t q_sh, const void* k_new, int64_t kn_sb, int64_t kn_sh,
                           const void* v_new, int64_t vn_sb, int64_t vn_sh, uint8_t* k_store, const kvq_strides_t* k_st,
                           float* k_scales, int k_bits, uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales,
                           int v_bits, void* out, int64_t o_sb, int64_t o_sh, int dtype, float sm_scale, int64_t window, float eps,
                           float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* d, void* stream) {
  KVQ_DECODE_CALL("kvq_decode_step_window");
  c.eps = eps;
  c.window = window;
  return decode_step_impl(c);
}

int kvq_decode_step_padded(const void* q, int64_t q_sb, int64_t q_sh, const void* k_new, int64_t kn_sb, int64_t kn_sh,
                           const void* v_new, int64_t vn_sb, int64_t vn_sh, uint8_t* k_store, const kvq_strides_t* k_st,
                           float* k_scales, int k_bits, uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales,
                           int v_bits, void* out, int64_t o_sb, int64_t o_sh, int dtype, float sm_scale, int64_t window,
                           const int32_t* kv_start, float eps, float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* d,
                           void* stream) {
  KVQ_DECODE_CALL(kv_start ? "kvq_decode_step_padded" : "kvq_decode_step_window");
  c.eps = eps;
  c.window = window;
  c.kv_start = kv_start;
  return decode_step_impl(c);
}

int kvq_decode_step_dev(const void* q, int64_t q_sb, int64_t q_sh, const void* k_new, int64_t kn_sb, int64_t kn_sh,
                        const void* v_new, int64_t vn_sb, int64_t vn_sh, uint8_t* k_store, const kvq_strides_t* k_st,
                        float* k_scales, int k_bits, uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales,
                        int v_bits, void* out, int64_t o_sb, int64_t o_sh, int dtype, float sm_scale, float eps,
                        float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* d, const int32_t* t_dev,
                        void* stream) {
  KVQ_DECODE_CALL("kvq_decode_step_dev");
  c.eps = eps;
  c.t_dev = t_dev;
  return decode_step_dev_impl(c);
}

int kvq_decode_step_dev_window(const void* q, int64_t q_sb, int64_t q_sh, const void* k_new, int64_t kn_sb, int64_t kn_sh,
                               const void* v_new, int64_t vn_sb, int64_t vn_sh, uint8_t* k_store, const kvq_strides_t* k_st,
                               float* k_scales, int k_bits, uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales,
                               int v_bits, void* out, int64_t o_sb, int64_t o_sh, int dtype, float sm_scale, int64_t window,
                               float eps, float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* d,
                               const int32_t* t_dev, void* stream) {
  KVQ_DECODE_CALL("kvq_decode_step_dev_window");
  c.eps = eps;
  c.window = window;
  c.t_dev = t_dev;
  return decode_step_dev_impl(c);
}

int kvq_decode_step_dev_padded(const void* q, int64_t q_sb, int64_t q_sh, const void* k_new, int64_t kn_sb, int64_t kn_sh,
                               const void* v_new, int64_t vn_sb, int64_t vn_sh, uint8_t* k_store, const kvq_strides_t* k_st,
                               float* k_scales, int k_bits, uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales,
                               int v_bits, void* out, int64_t o_sb, int64_t o_sh, int dtype, float sm_scale, int64_t window,
                               const int32_t* kv_start, float eps, float* workspace, int64_t workspace_floats,
                               const kvq_attn_dims_t* d, const int32_t* t_dev, void* stream) {
  KVQ_DECODE_CALL(kv_start ? "kvq_decode_step_dev_padded" : "kvq_decode_step_dev_window");
  c.eps = eps;
  c.window = window;
  c.kv_start = kv_start;
  c.t_dev = t_dev;
  return decode_step_dev_impl(c);
}

// The _ex entry points: the arguments of their _padded counterparts with window and kv_start in an options record, plus the
// two score modifiers. With both off the call IS the _padded call (same name in messages, same kernels, same bits).
#define KVQ_DECODE_OPTS(BASE)                                                                              \
  if (!opts) {                                                                                             \
    set_error(BASE "_ex: NULL opts");                                                                      \
    return KVQ_E_NULL;                                                                                     \
  }                                                                                                        \
  const bool mods = opts->softcap != 0.0f || opts->sinks;                                                  \
  KVQ_DECODE_CALL(mods ? BASE "_ex" : opts->kv_start ? BASE "_padded" : BASE "_window");                   \
  c.window = opts->window; c.kv_start = opts->kv_start; c.softcap = opts->softcap; c.sinks = opts->sinks

int kvq_decode_attn_ex(const void* q, int64_t q_sb, int64_t q_sh, const uint8_t* k_store, const kvq_strides_t* k_st,
                       const float* k_scales, int k_bits, const uint8_t* v_store, const kvq_strides_t* v_st,
                       const float* v_scales, int v_bits, const void* k_new, int64_t kn_sb, int64_t kn_sh,
                       const void* v_new, int64_t vn_sb, int64_t vn_sh, void* out, int64_t o_sb, int64_t o_sh, int dtype,
                       float sm_scale, const kvq_attn_opts_t* opts, float* workspace, int64_t workspace_floats,
                       const kvq_attn_dims_t* d, void* stream) {
  KVQ_DECODE_OPTS("kvq_decode_attn");
  // sinks alone without per-row starts keep the host-side window (the tuned partial kernels; only the merge changes)
  if (!padded_mode(c)) return decode_attn_window_impl(c);
  if (const int rc = check_window(c)) return rc;
  return decode_attn_impl(c, nullptr);
}

int kvq_decode_step_ex(const void* q, int64_t q_sb, int64_t q_sh, const void* k_new, int64_t kn_sb, int64_t kn_sh,
                       const void* v_new, int64_t vn_sb, int64_t vn_sh, uint8_t* k_store, const kvq_strides_t* k_st,
                       float* k_scales, int k_bits, uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales,
                       int v_bits, void* out, int64_t o_sb, int64_t o_sh, int dtype, float sm_scale,
                       const kvq_attn_opts_t* opts, float eps, float* workspace, int64_t workspace_floats,
                       const kvq_attn_dims_t* d, void* stream) {
  KVQ_DECODE_OPTS("kvq_decode_step");
  c.eps = eps;
  return decode_step_impl(c);
}

int kvq_decode_step_dev_ex(const void* q, int64_t q_sb, int64_t q_sh, const void* k_new, int64_t kn_sb, int64_t kn_sh,
                           const void* v_new, int64_t vn_sb, int64_t vn_sh, uint8_t* k_store, const kvq_strides_t* k_st,
                           float* k_scales, int k_bits, uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales,
                           int v_bits, void* out, int64_t o_sb, int64_t o_sh, int dtype, float sm_scale,
                           const kvq_attn_opts_t* opts, float eps, float* workspace, int64_t workspace_floats,
                           const kvq_attn_dims_t* d, const int32_t* t_dev, void* stream) {
  KVQ_DECODE_OPTS("kvq_decode_step_dev");
  c.eps = eps;
  c.t_dev = t_dev;
  return decode_step_dev_impl(c);
}

#undef KVQ_DECODE_OPTS
#undef KVQ_DECODE_CALL

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

// extend_kernel.inc — the extend kernel's text, included three times by extend.inc (the header there describes the tile walk and
// the two products): as extend_attn_k (KVQ_EXT_VARIANT 0: the kernel as it always was, token for token), as extend_attn_window_k
// (1: a sliding window) and as extend_attn_padded_k (2: a left-padded batch, with or without a window). One text, three kernels:
// compiled from a shared template body the unwindowed kernel did not stay instruction for instruction what it was, so the variant
// lines are cut in or out by the preprocessor instead. Where the variants differ the alternatives stand side by side under #if;
// each kernel's token stream is exactly what it was when the three were separate copies (tests/test_gpu_sliding_window.py
// ::test_extend_window_kernel_equals_extend_kernel still pins the same bits on the rows a window leaves whole).
//
// Window (1), launched only when the window of W keys cuts something. The host has moved the store to start at
// lo0 = max(0, T + 1 - W) (a.T = the tokens from there), so query row s sees stored t >= s - neg with neg = W - 1 - a.T >= 0, and
// chunk tokens s - W < j <= s. Stored and chunk tiles outside the window of every row of the workgroup are not walked (i_beg /
// j_beg: the first stored / chunk tile the workgroup's first chunk position sees); a split left with no visible token for a row
// writes m = -inf, l = 0, acc = 0 (the merge weighs it 0: every row sees its own chunk token).
//
// Padded (2), kvq_extend_attn_padded: the window kernel in ABSOLUTE key positions. Stored row t of the (host-shifted) store is key
// lo0 + t, chunk token j is key Tabs + j; the lower bound of query row s of batch row b is lb(s) = max(kv_start[b], T + s + 1 - W).
// Stored rows and chunk tokens before kv_start[b] are not read at all (the workgroup serves ONE batch row: they are staged as zero
// codes / zeros with scale 0), tiles before the bound of every row of the workgroup are not walked, and a row whose own position
// is padding sees no key: m = -inf, l = 0, acc = 0, which the single-split output path (l > 0 guard, this variant only) and
// extend_attn_merge_padded_k turn into zeros (extend_attn_merge_k would divide 0 by 0).
//
// Mod (3), extend_attn_mod_k (kvq_extend_attn_ex with a soft cap or sinks): the padded text with one more argument (AttnMod) and a
// NULL kv_start read as 0, so that the one form serves plain, windowed and padded calls. Soft cap: every scaled score, stored or
// chunk, becomes c tanh(s / c) (log2 domain) before the masks. Sinks: the single-split output path adds the row's head's sink as
// one more softmax term without a value row (M' = max(m, sink), l' = l 2^(m - M') + 2^(sink - M')); with several splits the merge
// (extend_attn_merge_mod_k) adds it, once.
template <int KBITS, int VBITS, int HD, int DT>
#if KVQ_EXT_VARIANT == 3
__global__ __launch_bounds__(256) void extend_attn_mod_k(const ExtendArgs a, const uint32_t W, const uint32_t lo0, const int32_t* kv_start, const AttnMod mod) {
#elif KVQ_EXT_VARIANT == 2
__global__ __launch_bounds__(256) void extend_attn_padded_k(const ExtendArgs a, const uint32_t W, const uint32_t lo0, const int32_t* kv_start) {
#elif KVQ_EXT_VARIANT == 1
__global__ __launch_bounds__(256) void extend_attn_window_k(const ExtendArgs a, const uint32_t W, const uint32_t neg) {
#else
__global__ __launch_bounds__(256) void extend_attn_k(const ExtendArgs a) {
#endif
  static_assert(HD == 64 || HD == 128, "head_dim of the extend kernel");
  constexpr int KS = HD / 32;                // k-steps of the score product
  constexpr int DB = HD / 16;                // 16-wide d blocks of the output
  constexpr int KLD = HD + 8;                // K image row, 2-byte elements (16-byte aligned rows, 4-bank shift per row)
  constexpr int VLD = kExtTC + 8;            // V^T image row
  constexpr int UPR = HD / 16;               // 16-element code units per token row
  constexpr int SU = kExtTC * UPR / 256;     // code units per thread and tile: 1 or 2
  constexpr int NPR = HD / 8;                // 8-element pieces per new-token row
  constexpr int NU = kExtTC * NPR / 256;     // pieces per thread and tile: 2 or 4
  constexpr uint32_t kZeroK = KBITS == 8 ? 0u : 0x88888888u;  // the code of 0
  constexpr uint32_t kZeroV = VBITS == 8 ? 0u : 0x88888888u;
  __shared__ __attribute__((aligned(16))) uint16_t s_k[kExtTC * KLD];
  __shared__ __attribute__((aligned(16))) uint16_t s_vt[HD * VLD];
  __shared__ float s_sk[kExtTC], s_sv[kExtTC];

  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6, x = lane & 15u, g = lane >> 4;
  const uint32_t qb = blockIdx.x, sp = blockIdx.y, bk = blockIdx.z;
  const uint32_t b = bk / a.Hkv, hk = bk - b * a.Hkv;
#if KVQ_EXT_VARIANT >= 2
  // absolute key positions: stored row t of the (host-shifted) store is key lo0 + t, chunk token j is key Tabs + j. This batch
  // row's start, clamped to [0, Tabs + S]; lower bound of chunk position s: lb(s) = max(start, Tabs + s + 1 - W)
  const uint32_t Tabs = lo0 + a.T;
#if KVQ_EXT_VARIANT == 3
  const int32_t ks_raw = kv_start ? *reinterpret_cast<const __attribute__((address_space(4))) int32_t*>(reinterpret_cast<uintptr_t>(kv_start) + 4u * (uintptr_t)b) : 0;
  const bool capped = mod.softcap > 0.f;  // uniform
  const Cap2 cap = cap_log2(mod);
#else
  const int32_t ks_raw = *reinterpret_cast<const __attribute__((address_space(4))) int32_t*>(reinterpret_cast<uintptr_t>(kv_start) + 4u * (uintptr_t)b);
#endif
  const uint32_t kstart = ks_raw < 0 ? 0u : ((uint32_t)ks_raw < Tabs + a.S ? (uint32_t)ks_raw : Tabs + a.S);
  auto lb = [&](const uint32_t s) -> uint32_t {
    const uint32_t wl = (W && Tabs + s + 1u > W) ? Tabs + s + 1u - W : 0u;
    return wl > kstart ? wl : kstart;
  };
#endif

  // this lane's query row (padding rows beyond M compute on zeros as chunk position S - 1 and are never written)
  const uint32_t row = qb * kExtQB + w * 16u + x;
  const bool row_ok = row < a.M;
  const uint32_t s_row = row_ok ? row / a.nq : a.S - 1u;
  const uint32_t h_row = row_ok ? row - s_row * a.nq : 0u;
  u32x4 qf[KS];
  if (row_ok) {
    const uint16_t* qp = reinterpret_cast<const uint16_t*>(a.q) + (int64_t)b * a.q_sb + (int64_t)(hk * a.nq + h_row) * a.q_sh +
                         (int64_t)s_row * a.q_ss + 8u * g;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const u32x4*>(qp + 32 * ks);
  } else {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = u32x4{0u, 0u, 0u, 0u};
  }
  const uint32_t m_end = a.M < qb * kExtQB + kExtQB ? a.M : qb * kExtQB + kExtQB;
  const uint32_t s_blk = (m_end - 1u) / a.nq;  // last chunk position of the workgroup's rows
  const uint32_t wrow0 = qb * kExtQB + w * 16u;
  const bool wave_live = wrow0 < a.M;
  const uint32_t s_wave = wave_live ? ((a.M < wrow0 + 16u ? a.M : wrow0 + 16u) - 1u) / a.nq : 0u;

  const uint32_t st0 = sp * a.tps * (uint32_t)kExtTC;
  const uint32_t st1 = st0 + a.tps * (uint32_t)kExtTC < a.T ? st0 + a.tps * (uint32_t)kExtTC : a.T;
  const uint32_t n_st = st1 > st0 ? (st1 - st0 + kExtTC - 1u) / kExtTC : 0u;
  const uint32_t n_new = sp == a.nsplit - 1u ? s_blk / kExtTC + 1u : 0u;
#if KVQ_EXT_VARIANT
  // the first stored / chunk tile inside the window of the workgroup's first chunk position (every later row's window starts
  // later): the tiles before them are not walked
  const uint32_t s_min = (qb * kExtQB) / a.nq;
#if KVQ_EXT_VARIANT >= 2
  const uint32_t lb_min = lb(s_min);  // the smallest lower bound of the workgroup's rows (lb is non-decreasing in s); >= lo0
  const uint32_t t_vis = lb_min > lo0 ? lb_min - lo0 : 0u;  // first stored row the workgroup's first chunk position sees
#else
  const uint32_t t_vis = s_min > neg ? s_min - neg : 0u;  // first stored token row s_min sees
#endif
  uint32_t i_beg = t_vis > st0 ? (t_vis - st0) / kExtTC : 0u;
  i_beg = i_beg < n_st ? i_beg : n_st;
#if KVQ_EXT_VARIANT >= 2
  const uint32_t j_vis = lb_min > Tabs ? lb_min - Tabs : 0u;  // first chunk token row s_min sees
  const uint32_t row_lb = lb(s_row);  // this lane's own lower bound
#else
  const uint32_t j_vis = s_min + 1u > W ? s_min + 1u - W : 0u;  // first chunk token row s_min sees
#endif
  const uint32_t j_beg = j_vis / kExtTC < n_new ? j_vis / kExtTC : n_new;
#endif
  const uint8_t* krow = a.k + (int64_t)b * a.k_sb + (int64_t)hk * a.k_sh;
  const uint8_t* vrow = a.v + (int64_t)b * a.v_sb + (int64_t)hk * a.v_sh;

  // the next stored tile, in registers
  Raw16<KBITS> kr[SU];
  Raw16<VBITS> vr[SU];
  float skr = 0.f, svr = 0.f;
  auto load_stored = [&](const uint32_t it) {
    const uint32_t t0 = st0 + it * kExtTC;
#pragma unroll
    for (int i = 0; i < SU; ++i) {
      const uint32_t u = tid + 256u * i, o = u / UPR, c = u - o * UPR, t = t0 + o;
#if KVQ_EXT_VARIANT >= 2
      if (t < st1 && lo0 + t >= kstart) {  // rows before this batch row's start are never read: zero codes
#else
      if (t < st1) {
#endif
        kr[i].load(krow + (int64_t)t * a.k_st + c * Raw16<KBITS>::kBytes);
        vr[i].load(vrow + (int64_t)t * a.v_st + c * Raw16<VBITS>::kBytes);
      } else {
        if constexpr (KBITS == 8) kr[i].w = u32x4{kZeroK, kZeroK, kZeroK, kZeroK};
        else kr[i].w = u32x2{kZeroK, kZeroK};
        if constexpr (VBITS == 8) vr[i].w = u32x4{kZeroV, kZeroV, kZeroV, kZeroV};
        else vr[i].w = u32x2{kZeroV, kZeroV};
      }
    }
    if (tid < (uint32_t)kExtTC) {
      const uint32_t t = t0 + tid;
#if KVQ_EXT_VARIANT >= 2
      const bool live = t < st1 && lo0 + t >= kstart;  // scales past the split's tokens or before the row's start are never read
      skr = live ? a.k_scale[t] : 0.f;
      svr = live ? a.v_scale[t] : 0.f;
#else
      skr = t < st1 ? a.k_scale[t] : 0.f;  // scales past the split's tokens are never read
      svr = t < st1 ? a.v_scale[t] : 0.f;
#endif
    }
  };
  auto narrow1 = [](const float v) -> uint16_t { return (uint16_t)(Elem<DT>::pack2(v, 0.f) & 0xFFFFu); };
  auto stage_stored = [&]() {
#pragma unroll
    for (int i = 0; i < SU; ++i) {
      const uint32_t u = tid + 256u * i, o = u / UPR, c = u - o * UPR;
      float kv[16], vv[16];
      kr[i].to_f32_biased(kv);
      vr[i].to_f32_biased(vv);
      constexpr float kb = Raw16<KBITS>::kBias, vb = Raw16<VBITS>::kBias;
      u32x4 w0, w1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        w0[j] = Elem<DT>::pack2(kv[2 * j] - kb, kv[2 * j + 1] - kb);
        w1[j] = Elem<DT>::pack2(kv[8 + 2 * j] - kb, kv[8 + 2 * j + 1] - kb);
      }
      *reinterpret_cast<u32x4*>(&s_k[o * KLD + c * 16u]) = w0;
      *reinterpret_cast<u32x4*>(&s_k[o * KLD + c * 16u + 8u]) = w1;
      const uint32_t pos = ext_vpos(o);
#pragma unroll
      for (int e = 0; e < 16; ++e) s_vt[(c * 16u + e) * VLD + pos] = narrow1(vv[e] - vb);
    }
    if (tid < (uint32_t)kExtTC) {
      s_sk[tid] = skr;
      s_sv[tid] = svr;
    }
  };
  // a tile of the exact new tokens: the values themselves, scale 1
  auto stage_new = [&](const uint32_t j0) {
    const uint16_t* knp = reinterpret_cast<const uint16_t*>(a.kn) + (int64_t)b * a.kn_sb + (int64_t)hk * a.kn_sh;
    const uint16_t* vnp = reinterpret_cast<const uint16_t*>(a.vn) + (int64_t)b * a.vn_sb + (int64_t)hk * a.vn_sh;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const uint32_t u = tid + 256u * i, o = u / NPR, c = u - o * NPR, j = j0 + o;
      u32x4 kw = {0u, 0u, 0u, 0u}, vw = {0u, 0u, 0u, 0u};
#if KVQ_EXT_VARIANT >= 2
      if (j < a.S && Tabs + j >= kstart) {  // chunk tokens before this batch row's start are never read: zeros
#else
      if (j < a.S) {
#endif
        kw = *reinterpret_cast<const u32x4*>(knp + (int64_t)j * a.kn_ss + 8u * c);
        vw = *reinterpret_cast<const u32x4*>(vnp + (int64_t)j * a.vn_ss + 8u * c);
      }
      *reinterpret_cast<u32x4*>(&s_k[o * KLD + c * 8u]) = kw;
      const uint32_t pos = ext_vpos(o);
#pragma unroll
      for (int e = 0; e < 8; ++e) s_vt[(c * 8u + e) * VLD + pos] = (uint16_t)((vw[e >> 1] >> (16 * (e & 1))) & 0xFFFFu);
    }
    if (tid < (uint32_t)kExtTC) {
#if KVQ_EXT_VARIANT >= 2
      const float one = (j0 + tid < a.S && Tabs + j0 + tid >= kstart) ? 1.f : 0.f;
#else
      const float one = j0 + tid < a.S ? 1.f : 0.f;
#endif
      s_sk[tid] = one;
      s_sv[tid] = one;
    }
  };

  float m = -INFINITY, l = 0.f, svref = 0.f;
  f32x4 acc[DB];
#pragma unroll
  for (int n = 0; n < DB; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

#if KVQ_EXT_VARIANT
  // loop index it walks stored tiles [i_beg, n_st), then chunk tiles j_beg ... (it - n_st + j_beg)
  const uint32_t ntile = n_st + n_new - j_beg;
  if (i_beg < n_st) load_stored(i_beg);
  for (uint32_t it = i_beg; it < ntile; ++it) {
    const bool is_new = it >= n_st;
    const uint32_t t0 = is_new ? (it - n_st + j_beg) * kExtTC : st0 + it * kExtTC;  // chunk position / stored token of tile row 0
#else
  const uint32_t ntile = n_st + n_new;
  if (n_st) load_stored(0u);
  for (uint32_t it = 0; it < ntile; ++it) {
    const bool is_new = it >= n_st;
    const uint32_t t0 = is_new ? (it - n_st) * kExtTC : st0 + it * kExtTC;  // chunk position / stored token of tile row 0
#endif
    if (is_new) stage_new(t0);
    else stage_stored();
    __syncthreads();
    if (it + 1u < n_st) load_stored(it + 1u);  // in flight while this tile is reduced
    const uint32_t nvalid = is_new ? 0u : (st1 - t0 < (uint32_t)kExtTC ? st1 - t0 : (uint32_t)kExtTC);
#if KVQ_EXT_VARIANT
    const uint32_t s_wmin = wrow0 / a.nq;  // first chunk position of the wave's rows
    // the tile lies before the window of every row of the wave
#if KVQ_EXT_VARIANT >= 2
    const bool w_out = (is_new ? Tabs : lo0) + t0 + (uint32_t)kExtTC - 1u < lb(s_wmin);
#else
    const bool w_out = is_new ? t0 + (uint32_t)kExtTC - 1u + W <= s_wmin : t0 + (uint32_t)kExtTC - 1u + neg < s_wmin;
#endif
    if (wave_live && !(is_new && t0 > s_wave) && !w_out) {
#else
    if (wave_live && !(is_new && t0 > s_wave)) {
#endif
      f32x4 sc[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        sc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
          sc[i] = ExtMfma<DT>::mma(*reinterpret_cast<const u32x4*>(&s_k[(16u * i + x) * KLD + 32u * ks + 8u * g]), qf[ks], sc[i]);
      }
      float p[4][4];
      float mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t o = 16u * i + 4u * g + r;
#if KVQ_EXT_VARIANT >= 2
          const bool ok = is_new ? t0 + o <= s_row && Tabs + t0 + o >= row_lb : o < nvalid && lo0 + t0 + o >= row_lb;
#elif KVQ_EXT_VARIANT == 1
          const bool ok = is_new ? t0 + o <= s_row && t0 + o + W > s_row : o < nvalid && t0 + o + neg >= s_row;
#else
          const bool ok = is_new ? t0 + o <= s_row : o < nvalid;
#endif
#if KVQ_EXT_VARIANT == 3
          const float s2 = sc[i][r] * s_sk[o] * a.scale_log2;
          p[i][r] = ok ? (capped ? softcap2(s2, cap) : s2) : -INFINITY;
#else
          p[i][r] = ok ? sc[i][r] * s_sk[o] * a.scale_log2 : -INFINITY;
#endif
          mx = fmaxf(mx, p[i][r]);
        }
      mx = xor32_max(xor16_max(mx));
      const float m_new = fmaxf(m, mx);
      const float m_use = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = exp2f(m - m_use);
      const float sv_new = fmaxf(svref, wave_fmax(s_sv[lane]));
      const float inv = sv_new > 0.f ? 1.f / sv_new : 0.f;
      const float f = sv_new > 0.f ? alpha * (svref * inv) : alpha;
      float lsum = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = exp2f(p[i][r] - m_use);
          lsum += e;
          p[i][r] = e * (s_sv[16u * i + 4u * g + r] * inv);
        }
      l = l * alpha + lsum;
      m = m_new;
      svref = sv_new;
#pragma unroll
      for (int n = 0; n < DB; ++n) acc[n] *= f;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const u32x4 pb = {Elem<DT>::pack2(p[2 * s][0], p[2 * s][1]), Elem<DT>::pack2(p[2 * s][2], p[2 * s][3]),
                          Elem<DT>::pack2(p[2 * s + 1][0], p[2 * s + 1][1]), Elem<DT>::pack2(p[2 * s + 1][2], p[2 * s + 1][3])};
#pragma unroll
        for (int n = 0; n < DB; ++n)
          acc[n] = ExtMfma<DT>::mma(*reinterpret_cast<const u32x4*>(&s_vt[(16u * n + x) * VLD + 32u * s + 8u * g]), pb, acc[n]);
      }
    }
    __syncthreads();
  }

  l = xor32_add(xor16_add(l));
  if (!row_ok) return;
  if (a.nsplit == 1u) {
#if KVQ_EXT_VARIANT == 3
    float sc = l > 0.f ? svref / l : 0.f;  // a row that sees no key (its own position is padding): zeros
    if (mod.sinks) {  // the sink as one more term: by arithmetic a row that sees no key still writes zeros (acc = 0, l' = 1)
      const float sink2 = mod.sinks[hk * a.nq + h_row] * 1.44269504088896341f;
      const float M = fmaxf(m, sink2);
      const float e = exp2f(m - M);  // m = -inf: 0
      sc = svref * e / (l * e + exp2f(sink2 - M));
    }
#elif KVQ_EXT_VARIANT == 2
    const float sc = l > 0.f ? svref / l : 0.f;  // a row that sees no key (its own position is padding): zeros
#else
    const float sc = svref / l;
#endif
    uint16_t* op = reinterpret_cast<uint16_t*>(a.out) + (int64_t)b * a.o_sb + (int64_t)(hk * a.nq + h_row) * a.o_sh +
                   (int64_t)s_row * a.o_ss + 4u * g;
#pragma unroll
    for (int n = 0; n < DB; ++n)
      *reinterpret_cast<u32x2*>(op + 16 * n) = u32x2{Elem<DT>::pack2(acc[n][0] * sc, acc[n][1] * sc), Elem<DT>::pack2(acc[n][2] * sc, acc[n][3] * sc)};
    return;
  }
  const int64_t prow = ((int64_t)bk * a.nsplit + sp) * ((int64_t)a.nqb * kExtQB) + row;
  if (g == 0u) {
    a.ws[2 * prow] = m;
    a.ws[2 * prow + 1] = l;
  }
  float* ap = a.ws + a.acc_off + prow * HD + 4u * g;
#pragma unroll
  for (int n = 0; n < DB; ++n) *reinterpret_cast<f32x4*>(ap + 16 * n) = acc[n] * svref;
}

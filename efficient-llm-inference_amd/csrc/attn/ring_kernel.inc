// ring_kernel.inc — the ring kernel's text, included twice by ring.inc: as decode_attn_lds_mfma_k (KVQ_RING_PADDED 0: the kernel
// as it always was, token for token) and as decode_attn_lds_mfma_padded_k (KVQ_RING_PADDED 1: a left-padded batch, host or device
// count). One text, two kernels: compiled from a shared template body the unpadded kernel did not stay instruction for instruction
// what it was (operand order, schedule), so the padded lines are cut out by the preprocessor instead.
// KVQ_RING_PADDED 2: decode_attn_lds_mfma_mod_k, the soft-capped ring kernel of the kvq_*_ex calls — the padded text with one more
// argument (AttnMod), a NULL kv_start read as 0 and the capped instantiations of the tile reducers (AttnStream::consume<true> /
// consume_direct<true>): the one capped form serves plain, windowed, device-count and padded calls alike.
#if KVQ_RING_PADDED
// Every (batch row, kv head) spreads ITS live tiles, stored rows [padded_lo, count), over the launch's waves as the device-count
// instantiation does (ring_dev_tpw); waves past a row's live tiles exit before they request anything; rows before padded_lo are never read.
template <int KBITS, int VBITS, int TC, bool KI8, int NB, int TG = 1, int HD = 128>
#if KVQ_RING_PADDED == 2
__global__ __launch_bounds__(kWave, TC >= 64 ? 2 : 3) void decode_attn_lds_mfma_mod_k(const AttnArgs a, const uint32_t tpw_host, const AttnMod mod) {
  const Cap2 cap = cap_log2(mod);
#else
__global__ __launch_bounds__(kWave, TC >= 64 ? 2 : 3) void decode_attn_lds_mfma_padded_k(const AttnArgs a, const uint32_t tpw_host) {
#endif
  constexpr bool TDEV = true;  // the tile range is derived in the kernel, whether the count is the host's or a device word
#else
template <int KBITS, int VBITS, int TC, bool KI8, int NB, int TG = 1, int HD = 128, bool TDEV = false>
__global__ __launch_bounds__(kWave, TC >= 64 ? 2 : 3) void decode_attn_lds_mfma_k(const AttnArgs a, const uint32_t tpw_host) {
#endif
  // HD = 64 (round 4; INT8 keys only: 64-byte key rows = the 4-chunk image of INT4 keys at head_dim 128; values of 64 / 32
  // bytes per row): a 64-token tile is 4 + 2 (INT4 values) or 4 + 4 requests of 1 KiB + the two scale rows, a ring slot 6.5 / 8.5 KiB
  static_assert(HD == 128 || (HD == 64 && KBITS == 8), "head_dim 128, or 64 with INT8 keys");
  typedef AttnStream<KBITS, VBITS, TC, HD, KI8, false, TG> ST;
  typedef __attribute__((address_space(3))) void* lds_ptr;
  constexpr int DVN = ST::DVN;
  static_assert(ST::CBK == 16, "16-byte K fragments (head_dim 128, or 64 with INT8 keys)");
  constexpr int KROW = HD * KBITS / 8, VROW = HD * VBITS / 8;   // stored bytes per token row
  constexpr int KCPR = KROW / 16, VCPR = VROW / 16;              // 16-byte chunks per row
  constexpr int KOPS = TC * KROW / 1024, VOPS = TC * VROW / 1024;  // 1 KiB wave requests per tile
  constexpr int OPS = KOPS + VOPS + 2;                           // + the two scale rows
  constexpr int SLOT = TC * (KROW + VROW) + 512;                 // K image, V image, 64 + 64 scale floats
  static_assert(NB >= 1 && OPS * (NB - 1) < 64, "the ring's requests must fit the vmcnt counter");
  extern __shared__ __attribute__((aligned(16))) uint8_t ring[];  // NB slots
  __shared__ __attribute__((aligned(16))) float s_ks[TC];
  __shared__ __attribute__((aligned(16))) float s_vs[TC];
  __shared__ __attribute__((aligned(16))) float s_al[16];
  const uint32_t lane = threadIdx.x, x = lane & 15u, g = lane >> 4;
  const uint32_t split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  // TDEV (its own instantiation: the host-count kernel stays instruction for instruction what it was): the count is the device
  // word of a graph-replayed step, clamped to the host's bound
  // (in the padded kernel TDEV is a constant true: there the count is live_tokens() — the host's T or the device word — and the
  // tile range is always derived here, per batch row, from padded_lo)
  uint32_t T = a.T;
  uint32_t lo = 0u;  // a sliding window under the device-side count: the first visible stored row (window_lo), T the count from it
#if KVQ_RING_PADDED
  T = live_tokens(a);
#if KVQ_RING_PADDED == 2
  lo = padded_lo(a, T, a.kv_start ? kv_start_of(a, b) : 0, a.kn != nullptr);
#else
  lo = padded_lo(a, T, kv_start_of(a, b), a.kn != nullptr);  // this batch row's first visible stored token
#endif
  T -= lo;
#else
  if constexpr (TDEV) {
    T = live_tokens(a);
    lo = window_lo(a, T);
    T -= lo;
  }
#endif
  const uint32_t ntiles = (T + (uint32_t)TC - 1u) / (uint32_t)TC;
  // which tiles are this wave's: a contiguous run of tpw tiles (a.lds != 3), or every nsplit-th tile (a.lds == 3: the
  // waves of a (batch row, kv head) then read ADJACENT tiles at about the same time, as neighbouring workgroups of the
  // dequantise kernels do; the online softmax does not care about the order)
  const bool strided = a.lds == 3u;
  // a device-side count: the live tiles spread over all the launch's waves (ring_dev_tpw: the merge derives the same split size)
  uint32_t tpw = tpw_host;
  if constexpr (TDEV) tpw = ring_dev_tpw(a, T, (uint32_t)TC);
  const uint32_t first = strided ? split : split * tpw;
  if constexpr (TDEV) {
    if (first >= ntiles) return;  // no tokens here at this count: the merge skips the split, nothing is requested
  }
  const uint32_t step = strided ? a.nsplit : 1u;
  uint32_t n;
  if (strided) n = first < ntiles ? (ntiles - first + step - 1u) / step : 0u;
  else n = (first + tpw < ntiles ? first + tpw : ntiles) - first;  // host: first < ntiles for every split
  const uint8_t* k_row0 = a.k + (int64_t)b * a.k_sb + (int64_t)hk * a.k_sh + (int64_t)lo * a.k_st;
  const uint8_t* v_row0 = a.v + (int64_t)b * a.v_sb + (int64_t)hk * a.v_sh + (int64_t)lo * a.v_st;
  const float* k_scale0 = a.k_scale + lo;
  const float* v_scale0 = a.v_scale + lo;

  // per-lane source offsets of the K requests: request j covers rows (1024 / KROW) j ..., lane l = slot l % KCPR of row
  // l / KCPR; it fetches chunk slot ^ f(row). f depends on j only through its parity (INT8) or not at all (INT4).
  uint32_t k_off[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const uint32_t row = (uint32_t)par * (1024u / KROW) + lane / KCPR;
    k_off[par] = (lane / KCPR) * (uint32_t)a.k_st + (((lane % KCPR) ^ k_swizzle<KCPR>(row)) << 4);
  }
  const uint32_t v_off = (lane / VCPR) * (uint32_t)a.v_st + ((lane % VCPR) << 4);

  auto request = [&](const uint32_t k) {  // tile k of this wave -> ring slot k % NB; nothing waits here
    const uint32_t tt = first + (k < n ? k : 0u) * step;
    const uint32_t t0 = tt * (uint32_t)TC;
    const uint32_t cnt = k < n ? (T - t0 < (uint32_t)TC ? T - t0 : (uint32_t)TC) : 0u;  // 0: empty descriptors, no traffic
    uint8_t* slot = ring + (k % NB) * SLOT;
    const __amdgpu_buffer_rsrc_t kr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(k_row0 + (int64_t)t0 * a.k_st), 0, (int)(cnt * (uint32_t)a.k_st), 0x00020000);
    const __amdgpu_buffer_rsrc_t vr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(v_row0 + (int64_t)t0 * a.v_st), 0, (int)(cnt * (uint32_t)a.v_st), 0x00020000);
    const __amdgpu_buffer_rsrc_t ksr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(k_scale0 + t0), 0, (int)(cnt * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t vsr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(v_scale0 + t0), 0, (int)(cnt * 4u), 0x00020000);
#pragma unroll
    for (int j = 0; j < KOPS; ++j)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(kr, (lds_ptr)(slot + 1024 * j), 16, k_off[j & 1], (uint32_t)(j * (1024 / KROW)) * (uint32_t)a.k_st, 0, kKvAux);
#pragma unroll
    for (int j = 0; j < VOPS; ++j)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(vr, (lds_ptr)(slot + TC * KROW + 1024 * j), 16, v_off, (uint32_t)(j * (1024 / VROW)) * (uint32_t)a.v_st, 0, kKvAux);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(ksr, (lds_ptr)(slot + TC * (KROW + VROW)), 4, lane * 4u, 0, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(vsr, (lds_ptr)(slot + TC * (KROW + VROW) + 256), 4, lane * 4u, 0, 0, 0);
  };

  ST st;
  constexpr int PRE = NB > 1 ? NB - 1 : 1;  // tiles requested before the loop
#pragma unroll
  for (int k = 0; k < PRE; ++k) request((uint32_t)k);
  st.init(a, b, hk);
  if constexpr (TG == 4) {
    // the largest V scale of the wave's own tokens, once: consume_direct's fixed reference (P is carried as p sv / svref <= 1)
    float vm = 0.0f;
    if (!strided) {
      const uint32_t tok0 = first * (uint32_t)TC;
      const uint32_t cnt = T - tok0 < n * (uint32_t)TC ? T - tok0 : n * (uint32_t)TC;
      const __amdgpu_buffer_rsrc_t vsr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(v_scale0 + tok0), 0, (int)(cnt * 4u), 0x00020000);
      for (uint32_t i0 = 0; i0 < cnt; i0 += 1024u) {  // 256 floats per wave load, four loads in flight
        u32x4 w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = __builtin_amdgcn_raw_buffer_load_b128(vsr, (i0 + 256u * j + 4u * lane) * 4u, 0, 0);  // past cnt: zeros
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) vm = fmaxf(vm, __uint_as_float(w[j][e]));
      }
    } else {
      for (uint32_t k = 0; k < n; ++k) {
        const uint32_t t = (first + k * step) * (uint32_t)TC + lane;
        if (t < T) vm = fmaxf(vm, v_scale0[t]);
      }
    }
    vm = wave_fmax(vm);
    st.svref = vm;
    st.svn = vm > 0.0f ? 1.0f / vm : 0.0f;
  }
  typename ST::Raw r;
  const typename ST::Src none = st.src(a, b, hk, 0u, 0u);
  for (uint32_t k = 0; k < n; ++k) {
    if constexpr (NB > 1) {
      // the slot tile k + NB - 1 goes to is the one tile k - 1 was read from: those reads have all been consumed
      // (their values fed MFMAs of the previous iteration); the compiler is kept from moving anything across
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      request(k + (uint32_t)(NB - 1));
      wait_vmcnt<OPS * (NB - 1)>();  // tile k has landed
    } else {
      wait_vmcnt<0>();  // ONE slot: tile k has landed; the next request goes out as soon as its bytes are in registers
    }
    asm volatile("" ::: "memory");
    const uint32_t t0 = (first + k * step) * (uint32_t)TC;
    const uint32_t nt = T - t0 < (uint32_t)TC ? T - t0 : (uint32_t)TC;
    const uint8_t* slot = ring + (k % NB) * SLOT;
    read_fragments<KBITS, VBITS, TC, KI8, typename ST::Raw, HD>(slot, r);
    static_assert(TC <= kWave, "one scale per lane");
    const float* sc = reinterpret_cast<const float*>(slot + TC * (KROW + VROW));
    if constexpr (TG == 4 && NB > 1) {
#if KVQ_RING_PADDED == 2
      st.template consume_direct<true>(a, nt, r, sc, cap);
#else
      st.consume_direct(a, nt, r, sc);
#endif
      continue;
    }
    const float ksv = sc[lane < (uint32_t)TC ? lane : 0u], vsv = sc[64 + (lane < (uint32_t)TC ? lane : 0u)];
    r.ks[0] = lane < nt ? ksv : 0.0f;  // rows past nt: the request's range check left the slot's old bytes there
    r.vs[0] = lane < nt ? vsv : 0.0f;
    if constexpr (NB == 1) {
      // every fragment is in registers once the LDS reads have returned: the slot is free for tile k + 1, whose
      // requests then have the whole reduction of tile k to land in
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(r.ks[0]), "+v"(r.vs[0]) : : "memory");
      request(k + 1u);
      asm volatile("" ::: "memory");
    }
#if KVQ_RING_PADDED == 2
    st.template consume<true>(a, nt, r, none, s_ks, s_vs, s_al, cap);
#else
    st.consume(a, nt, r, none, s_ks, s_vs, s_al);
#endif
  }
  wait_vmcnt<0>();  // the empty tail requests retire before the wave's LDS is released
  if constexpr (TG == 4 && NB > 1) st.reduce_l();
  // ---- workspace: (m, l) per head, acc[heads][D] — the layout the merge kernels read ---------------------------
  if (g == 0u && x < a.nq) {
    const int64_t oi = (((int64_t)b * a.Hq + hk * a.nq + x) * a.nsplit + split) * 2;
    a.ws[oi] = st.m * 0.693147180559945309f;
    a.ws[oi + 1] = st.l;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t h = 4 * g + q;
    if (h < a.nq) {
      float o8[DVN];
#pragma unroll
      for (int c = 0; c < DVN; ++c) {
        int e = c;
        if constexpr (VBITS == 4 && HD == 128) e = c < 4 ? 2 * c : 2 * (c - 4) + 1;
        if constexpr (VBITS == 4 && HD == 64) e = c == 1 ? 2 : (c == 2 ? 1 : c);
        o8[e] = st.acc[c][q] * st.svref;
      }
      const int64_t di = a.acc_off + (((int64_t)b * a.Hq + hk * a.nq + h) * a.nsplit + split) * a.D + DVN * x;
#pragma unroll
      for (int c = 0; c < DVN; c += 4) *reinterpret_cast<f32x4*>(a.ws + di + c) = f32x4{o8[c], o8[c + 1], o8[c + 2], o8[c + 3]};
    }
  }
}

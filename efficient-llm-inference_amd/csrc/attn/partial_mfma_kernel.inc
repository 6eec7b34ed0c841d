// partial_mfma_kernel.inc — the one-tile MFMA partial kernel's text (a wrapper around AttnTile::run), included three times by
// tile_mfma.inc: as decode_attn_partial_mfma_k (KVQ_PARTIAL_VARIANT 0: the host-count kernel as it always was, token for token), as
// decode_attn_partial_mfma_window_k (1: a device-side count with a sliding window) and as decode_attn_partial_mfma_padded_k (2: a
// left-padded batch, host or device count). The variants differ only in where the split's rows start and how many are live:
//   0  T = live_tokens; the rows start at the store's row 0
//   1  the rows start lo = window_lo rows into the store, T = the count from there (live_window)
//   2  the rows start lo = padded_lo rows into the store, the larger of the window's bound and kv_start[b] of the workgroup's batch
//      row; a split past the row's live count exits before it requests anything
//   3  decode_attn_partial_mfma_mod_k (a soft-capped kvq_*_ex call): variant 2 with one more argument (AttnMod), the scores capped
//      in AttnTile::run<true>, and a NULL kv_start read as 0 — the one capped form serves plain, windowed, device-count and padded calls
// (tests/test_gpu_sliding_window.py::test_device_count_window_kernels_equal_unwindowed asserts the same bits from 0 and 1 on a
// window that cuts nothing.)
template <int KBITS, int VBITS, int TC, int HD, bool KI8 = false>
#if KVQ_PARTIAL_VARIANT == 3
__global__ __launch_bounds__(kWave) void decode_attn_partial_mfma_mod_k(const AttnArgs a, const AttnMod mod) {
#elif KVQ_PARTIAL_VARIANT == 2
__global__ __launch_bounds__(kWave) void decode_attn_partial_mfma_padded_k(const AttnArgs a) {
#elif KVQ_PARTIAL_VARIANT == 1
__global__ __launch_bounds__(kWave) void decode_attn_partial_mfma_window_k(const AttnArgs a) {
#else
__global__ __launch_bounds__(kWave) void decode_attn_partial_mfma_k(const AttnArgs a) {
#endif
  typedef AttnTile<KBITS, VBITS, TC, HD, KI8> Tile;
  constexpr int DVN = Tile::DVN;
  __shared__ __attribute__((aligned(16))) float s_ks[TC];
  __shared__ __attribute__((aligned(16))) float s_vs[TC];
  const uint32_t lane = threadIdx.x;
  const uint32_t x = lane & 15u, g = lane >> 4;
  const uint32_t split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const uint32_t t0 = split * TC;
#if KVQ_PARTIAL_VARIANT >= 2
  const uint32_t t = live_tokens(a);
#if KVQ_PARTIAL_VARIANT == 3
  const uint32_t lo = padded_lo(a, t, a.kv_start ? kv_start_of(a, b) : 0, a.kn != nullptr);
#else
  const uint32_t lo = padded_lo(a, t, kv_start_of(a, b), a.kn != nullptr);  // padded: this row's first visible stored token
#endif
  const uint32_t T = t - lo;
  if (t0 >= T) return;  // nothing of this row's live tokens in this split
#elif KVQ_PARTIAL_VARIANT == 1
  uint32_t lo;  // window: the split's tokens start lo rows into the store
  const uint32_t T = live_window(a, lo);
  if (t0 >= T) return;  // device-side T (graph replay): this split holds nothing yet
#else
  const uint32_t T = live_tokens(a);
  if (t0 >= T) return;  // device-side T (graph replay): this split holds nothing yet
#endif
  const uint32_t nt = T - t0 < (uint32_t)TC ? T - t0 : (uint32_t)TC;
  Tile tile;
#if KVQ_PARTIAL_VARIANT == 3
  tile.template run<true>(a, b, hk, t0 + lo, nt, s_ks, s_vs, cap_log2(mod));
#elif KVQ_PARTIAL_VARIANT
  tile.run(a, b, hk, t0 + lo, nt, s_ks, s_vs);
#else
  tile.run(a, b, hk, t0, nt, s_ks, s_vs);
#endif
  // ---- workspace: (m, l) per head, acc[heads][D] --------------------------------------------------
  if (g == 0u && x < a.nq) {
    float* o = a.ws + (((int64_t)b * a.Hq + hk * a.nq + x) * a.nsplit + split) * 2;
    o[0] = tile.m * 0.693147180559945309f;  // back to the natural-log domain the merge kernel works in
    o[1] = tile.l;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t h = 4 * g + r;
    if (h < a.nq) {
      float o8[DVN];
      tile.ordered(r, tile.svmax, o8);
      float* dst = a.ws + a.acc_off + (((int64_t)b * a.Hq + hk * a.nq + h) * a.nsplit + split) * a.D + DVN * x;
#pragma unroll
      for (int c = 0; c < DVN; c += 4) *reinterpret_cast<f32x4*>(dst + c) = f32x4{o8[c], o8[c + 1], o8[c + 2], o8[c + 3]};
    }
  }
}

// extend_merge_kernel.inc — the extend merge's text, included twice by extend.inc: as extend_attn_merge_k (KVQ_EXT_MERGE_PADDED 0:
// the kernel as it always was, token for token) and as extend_attn_merge_padded_k (1: a left-padded batch, where a row whose own
// position is padding has l = 0 and m = -inf in every split and writes zeros; the unpadded kernel would divide 0 by 0).
// one wave per query row: out = sum_i e^(m_i - M) acc_i / sum_i e^(m_i - M) l_i over the splits (log2 domain)
// KVQ_EXT_MERGE_PADDED 2: extend_attn_merge_mod_k (kvq_extend_attn_ex): the padded text with one more argument (AttnMod); the row's
// head's sink joins once, here, as one more term without a value row (log2 domain: sink log2(e)).
template <int HD, int DT>
#if KVQ_EXT_MERGE_PADDED == 2
__global__ __launch_bounds__(256) void extend_attn_merge_mod_k(const ExtendArgs a, const AttnMod mod) {
#elif KVQ_EXT_MERGE_PADDED
__global__ __launch_bounds__(256) void extend_attn_merge_padded_k(const ExtendArgs a) {
#else
__global__ __launch_bounds__(256) void extend_attn_merge_k(const ExtendArgs a) {
#endif
  constexpr int EPL = HD / 64;  // output elements per lane
  const uint32_t lane = threadIdx.x & 63u, row = blockIdx.x * 4u + (threadIdx.x >> 6), bk = blockIdx.y;
  if (row >= a.M) return;
  const uint32_t b = bk / a.Hkv, hk = bk - b * a.Hkv, s_row = row / a.nq, h_row = row - s_row * a.nq;
  const int64_t mp = (int64_t)a.nqb * kExtQB, base = (int64_t)bk * a.nsplit * mp + row;
  float mmax = -INFINITY;
  for (uint32_t sp = 0; sp < a.nsplit; ++sp) mmax = fmaxf(mmax, a.ws[2 * (base + sp * mp)]);
  float L = 0.f, o[EPL];
#if KVQ_EXT_MERGE_PADDED == 2
  if (mod.sinks) {
    const float sink2 = mod.sinks[hk * a.nq + h_row] * 1.44269504088896341f;
    mmax = fmaxf(mmax, sink2);
    L = exp2f(sink2 - mmax);
  }
#endif
#pragma unroll
  for (int k = 0; k < EPL; ++k) o[k] = 0.f;
  for (uint32_t sp = 0; sp < a.nsplit; ++sp) {
    const int64_t pr = base + sp * mp;
#if KVQ_EXT_MERGE_PADDED
    const float e = mmax == -INFINITY ? 0.f : exp2f(a.ws[2 * pr] - mmax);  // no split saw a key: weights 0
#else
    const float e = exp2f(a.ws[2 * pr] - mmax);
#endif
    L += a.ws[2 * pr + 1] * e;
    const float* ap = a.ws + a.acc_off + pr * HD + EPL * lane;
#pragma unroll
    for (int k = 0; k < EPL; ++k) o[k] += e * ap[k];
  }
#if KVQ_EXT_MERGE_PADDED
  const float inv = L > 0.f ? 1.f / L : 0.f;
#else
  const float inv = 1.f / L;
#endif
  uint16_t* op = reinterpret_cast<uint16_t*>(a.out) + (int64_t)b * a.o_sb + (int64_t)(hk * a.nq + h_row) * a.o_sh +
                 (int64_t)s_row * a.o_ss + EPL * lane;
  if constexpr (EPL == 2) *reinterpret_cast<uint32_t*>(op) = Elem<DT>::pack2(o[0] * inv, o[1] * inv);
  else *op = (uint16_t)(Elem<DT>::pack2(o[0] * inv, 0.f) & 0xFFFFu);
}

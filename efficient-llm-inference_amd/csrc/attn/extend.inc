// extend.inc — part of kvq_attn.hip (one translation unit, included last): multi-token causal attention over the quantised
// store (kvq_extend_attn): S new query tokens per (batch row, query head) attend the T stored tokens (INT8 / packed INT4 +
// per-token scales) and, causally, the S new tokens' exact K / V. Query row s sees stored tokens [0, T) and new tokens
// j <= s: HF's lower-right-aligned causal mask for a forward with T past tokens.
//
// extend_attn_k: grid (query block, split, batch row x kv head), 256 threads = 4 waves x 16 query rows. The query rows of a
//   kv head are (chunk position s, query head h) pairs, row = s * nq + h, so a block of 64 rows is a few consecutive chunk
//   positions of every query head of the kv head: the store is read ONCE for all of them (speculative verify: S * nq <= 64
//   rows is one block; chunked prefill: many blocks, the store's tiles shared through L2).
//   Per 64-token tile the workgroup converts the K / V codes EXACTLY to f16 / bf16 integers into LDS (K as [token][d], V
//   transposed [d][token] in the k order the P V product consumes) with the per-token scales beside them; the next stored
//   tile's bytes are requested before the current tile is reduced. Each wave then runs both products on the matrix cores
//   (v_mfma_f32_16x16x32_{f16,bf16}) with online softmax:
//     S^T = K Q^T   A = K rows (token x, k = d), B = Q (col = query row x): lane (x, g) holds query row x, tokens
//                   16 i + 4 g + r — the whole score row of a token set in the lane's registers, reduced across the four
//                   16-lane groups with lane swaps (no LDS)
//     O^T = V^T P^T B = P^T straight from the score registers (k order of a 32-token step: 32 s + 4 g + j, 32 s + 16 + 4 g +
//                   j - 4), A = V^T rows from LDS; lane (x, g) holds query row x, d = 16 n + 4 g + r
//   scores s = acc * sk[t] * sm_scale (the K scale factors out of the integer product). P is multiplied by sv[t] / svref
//   before it is rounded to f16 / bf16 (svref = running max of the V scales seen, so P' <= 1 and no underflow), the
//   accumulator is kept in units of svref. The new tokens are tiles with scale 1 that the LAST split walks after its stored
//   tiles, masked causally per row.
// extend_attn_merge_k: log-sum-exp merge of the splits (one wave per query row); a single split writes the output itself.
namespace kvq {

constexpr int kExtQB = 64;        // query rows per workgroup
constexpr int kExtTC = 64;        // tokens per tile
constexpr int kExtMaxSplit = 64;  // splits over the stored tokens
constexpr int kExtTargetWG = 1024;  // workgroups a launch aims for (4 per CU: 36 KiB of LDS each at head_dim 128)

struct ExtendArgs {
  const void* q;
  int64_t q_sb, q_sh, q_ss;  // elements
  const uint8_t* k;
  int64_t k_sb, k_sh, k_st;  // bytes
  const float* k_scale;
  const uint8_t* v;
  int64_t v_sb, v_sh, v_st;
  const float* v_scale;
  const void* kn;
  int64_t kn_sb, kn_sh, kn_ss;
  const void* vn;
  int64_t vn_sb, vn_sh, vn_ss;
  void* out;
  int64_t o_sb, o_sh, o_ss;
  float* ws;        // nsplit > 1: [B*Hkv][nsplit][nqb*64] (m, l), then at acc_off the same rows x D of acc
  int64_t acc_off;  // floats
  float scale_log2;  // sm_scale * log2(e)
  uint32_t B, Hkv, nq, T, S, M, nqb, nsplit, tps;  // M = S * nq rows per kv head; tps = stored tiles per split
};

template <int DT>
struct ExtMfma;
template <>
struct ExtMfma<KVQ_F16> {
  __device__ static inline f32x4 mma(const u32x4 a, const u32x4 b, const f32x4 c) {
    f16x8 ah, bh;
    __builtin_memcpy(&ah, &a, 16);
    __builtin_memcpy(&bh, &b, 16);
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, c, 0, 0, 0);
  }
};
template <>
struct ExtMfma<KVQ_BF16> {
  typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
  __device__ static inline f32x4 mma(const u32x4 a, const u32x4 b, const f32x4 c) {
    bf16x8 ah, bh;
    __builtin_memcpy(&ah, &a, 16);
    __builtin_memcpy(&bh, &b, 16);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, c, 0, 0, 0);
  }
};

// position of tile token o in a row of the transposed V image: the k order of the P V step (see the header)
__device__ inline uint32_t ext_vpos(const uint32_t o) {
  return (o & 32u) | (((o >> 2) & 3u) << 3) | (((o >> 4) & 1u) << 2) | (o & 3u);
}

// (extend_attn_window_k below is a copy of this body with a sliding window: a fix here belongs there too)
template <int KBITS, int VBITS, int HD, int DT>
__global__ __launch_bounds__(256) void extend_attn_k(const ExtendArgs a) {
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
      if (t < st1) {
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
      skr = t < st1 ? a.k_scale[t] : 0.f;  // scales past the split's tokens are never read
      svr = t < st1 ? a.v_scale[t] : 0.f;
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
      if (j < a.S) {
        kw = *reinterpret_cast<const u32x4*>(knp + (int64_t)j * a.kn_ss + 8u * c);
        vw = *reinterpret_cast<const u32x4*>(vnp + (int64_t)j * a.vn_ss + 8u * c);
      }
      *reinterpret_cast<u32x4*>(&s_k[o * KLD + c * 8u]) = kw;
      const uint32_t pos = ext_vpos(o);
#pragma unroll
      for (int e = 0; e < 8; ++e) s_vt[(c * 8u + e) * VLD + pos] = (uint16_t)((vw[e >> 1] >> (16 * (e & 1))) & 0xFFFFu);
    }
    if (tid < (uint32_t)kExtTC) {
      const float one = j0 + tid < a.S ? 1.f : 0.f;
      s_sk[tid] = one;
      s_sv[tid] = one;
    }
  };

  float m = -INFINITY, l = 0.f, svref = 0.f;
  f32x4 acc[DB];
#pragma unroll
  for (int n = 0; n < DB; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const uint32_t ntile = n_st + n_new;
  if (n_st) load_stored(0u);
  for (uint32_t it = 0; it < ntile; ++it) {
    const bool is_new = it >= n_st;
    const uint32_t t0 = is_new ? (it - n_st) * kExtTC : st0 + it * kExtTC;  // chunk position / stored token of tile row 0
    if (is_new) stage_new(t0);
    else stage_stored();
    __syncthreads();
    if (it + 1u < n_st) load_stored(it + 1u);  // in flight while this tile is reduced
    const uint32_t nvalid = is_new ? 0u : (st1 - t0 < (uint32_t)kExtTC ? st1 - t0 : (uint32_t)kExtTC);
    if (wave_live && !(is_new && t0 > s_wave)) {
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
          const bool ok = is_new ? t0 + o <= s_row : o < nvalid;
          p[i][r] = ok ? sc[i][r] * s_sk[o] * a.scale_log2 : -INFINITY;
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
    const float sc = svref / l;
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

// extend_attn_window_k: extend_attn_k under a sliding window of W keys, launched only when the window cuts something. The
// host has moved the store to start at lo0 = max(0, T + 1 - W) (a.T = the tokens from there), so query row s sees stored t >= s - neg with neg = W - 1 - a.T >= 0, and chunk tokens
// s - W < j <= s. Stored and chunk tiles outside the window of every row of the workgroup are not walked; a split left with
// no visible token for a row writes m = -inf, l = 0, acc = 0 (the merge weighs it 0: every row sees its own chunk token).
// (Its own copy of extend_attn_k's body: compiled from one shared body the unwindowed kernel did not stay instruction for
// instruction what it was. A fix to one body belongs in the other; tests/test_gpu_sliding_window.py
// ::test_extend_window_kernel_equals_extend_kernel asserts the same bits on the rows a window leaves whole.)
template <int KBITS, int VBITS, int HD, int DT>
__global__ __launch_bounds__(256) void extend_attn_window_k(const ExtendArgs a, const uint32_t W, const uint32_t neg) {
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
  // the first stored / chunk tile inside the window of the workgroup's first chunk position (every later row's window starts
  // later): the tiles before them are not walked
  const uint32_t s_min = (qb * kExtQB) / a.nq;
  const uint32_t t_vis = s_min > neg ? s_min - neg : 0u;  // first stored token row s_min sees
  uint32_t i_beg = t_vis > st0 ? (t_vis - st0) / kExtTC : 0u;
  i_beg = i_beg < n_st ? i_beg : n_st;
  const uint32_t j_vis = s_min + 1u > W ? s_min + 1u - W : 0u;  // first chunk token row s_min sees
  const uint32_t j_beg = j_vis / kExtTC < n_new ? j_vis / kExtTC : n_new;
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
      if (t < st1) {
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
      skr = t < st1 ? a.k_scale[t] : 0.f;  // scales past the split's tokens are never read
      svr = t < st1 ? a.v_scale[t] : 0.f;
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
      if (j < a.S) {
        kw = *reinterpret_cast<const u32x4*>(knp + (int64_t)j * a.kn_ss + 8u * c);
        vw = *reinterpret_cast<const u32x4*>(vnp + (int64_t)j * a.vn_ss + 8u * c);
      }
      *reinterpret_cast<u32x4*>(&s_k[o * KLD + c * 8u]) = kw;
      const uint32_t pos = ext_vpos(o);
#pragma unroll
      for (int e = 0; e < 8; ++e) s_vt[(c * 8u + e) * VLD + pos] = (uint16_t)((vw[e >> 1] >> (16 * (e & 1))) & 0xFFFFu);
    }
    if (tid < (uint32_t)kExtTC) {
      const float one = j0 + tid < a.S ? 1.f : 0.f;
      s_sk[tid] = one;
      s_sv[tid] = one;
    }
  };

  float m = -INFINITY, l = 0.f, svref = 0.f;
  f32x4 acc[DB];
#pragma unroll
  for (int n = 0; n < DB; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

  // loop index it walks stored tiles [i_beg, n_st), then chunk tiles j_beg ... (it - n_st + j_beg)
  const uint32_t ntile = n_st + n_new - j_beg;
  if (i_beg < n_st) load_stored(i_beg);
  for (uint32_t it = i_beg; it < ntile; ++it) {
    const bool is_new = it >= n_st;
    const uint32_t t0 = is_new ? (it - n_st + j_beg) * kExtTC : st0 + it * kExtTC;  // chunk position / stored token of tile row 0
    if (is_new) stage_new(t0);
    else stage_stored();
    __syncthreads();
    if (it + 1u < n_st) load_stored(it + 1u);  // in flight while this tile is reduced
    const uint32_t nvalid = is_new ? 0u : (st1 - t0 < (uint32_t)kExtTC ? st1 - t0 : (uint32_t)kExtTC);
    const uint32_t s_wmin = wrow0 / a.nq;  // first chunk position of the wave's rows
    // the tile lies before the window of every row of the wave
    const bool w_out = is_new ? t0 + (uint32_t)kExtTC - 1u + W <= s_wmin : t0 + (uint32_t)kExtTC - 1u + neg < s_wmin;
    if (wave_live && !(is_new && t0 > s_wave) && !w_out) {
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
          const bool ok = is_new ? t0 + o <= s_row && t0 + o + W > s_row : o < nvalid && t0 + o + neg >= s_row;
          p[i][r] = ok ? sc[i][r] * s_sk[o] * a.scale_log2 : -INFINITY;
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
    const float sc = svref / l;
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

// one wave per query row: out = sum_i e^(m_i - M) acc_i / sum_i e^(m_i - M) l_i over the splits (log2 domain)
template <int HD, int DT>
__global__ __launch_bounds__(256) void extend_attn_merge_k(const ExtendArgs a) {
  constexpr int EPL = HD / 64;  // output elements per lane
  const uint32_t lane = threadIdx.x & 63u, row = blockIdx.x * 4u + (threadIdx.x >> 6), bk = blockIdx.y;
  if (row >= a.M) return;
  const uint32_t b = bk / a.Hkv, hk = bk - b * a.Hkv, s_row = row / a.nq, h_row = row - s_row * a.nq;
  const int64_t mp = (int64_t)a.nqb * kExtQB, base = (int64_t)bk * a.nsplit * mp + row;
  float mmax = -INFINITY;
  for (uint32_t sp = 0; sp < a.nsplit; ++sp) mmax = fmaxf(mmax, a.ws[2 * (base + sp * mp)]);
  float L = 0.f, o[EPL];
#pragma unroll
  for (int k = 0; k < EPL; ++k) o[k] = 0.f;
  for (uint32_t sp = 0; sp < a.nsplit; ++sp) {
    const int64_t pr = base + sp * mp;
    const float e = exp2f(a.ws[2 * pr] - mmax);
    L += a.ws[2 * pr + 1] * e;
    const float* ap = a.ws + a.acc_off + pr * HD + EPL * lane;
#pragma unroll
    for (int k = 0; k < EPL; ++k) o[k] += e * ap[k];
  }
  const float inv = 1.f / L;
  uint16_t* op = reinterpret_cast<uint16_t*>(a.out) + (int64_t)b * a.o_sb + (int64_t)(hk * a.nq + h_row) * a.o_sh +
                 (int64_t)s_row * a.o_ss + EPL * lane;
  if constexpr (EPL == 2) *reinterpret_cast<uint32_t*>(op) = Elem<DT>::pack2(o[0] * inv, o[1] * inv);
  else *op = (uint16_t)(Elem<DT>::pack2(o[0] * inv, 0.f) & 0xFFFFu);
}

// extend_attn_padded_k: extend_attn_window_k for a left-padded batch (kvq_extend_attn_padded, with or without a window): the
// lower bound of query row s of batch row b is lb = max(kv_start[b], T + s + 1 - W) in absolute key positions (lo0 = where the
// host-shifted store starts, as for the window kernel). Stored rows and chunk tokens before kv_start[b] are not read at all
// (the workgroup serves ONE batch row: they are staged as zero codes / zeros with scale 0), tiles before the bound of every
// row of the workgroup are not walked, and a row whose own position is padding sees no key: m = -inf, l = 0, acc = 0, which
// the single-split output path and extend_attn_merge_padded_k turn into zeros (extend_attn_merge_k would divide 0 by 0).
// (A third copy of extend_attn_k's body, for the reason extend_attn_window_k gives: a fix to one body belongs in the others.)
template <int KBITS, int VBITS, int HD, int DT>
__global__ __launch_bounds__(256) void extend_attn_padded_k(const ExtendArgs a, const uint32_t W, const uint32_t lo0, const int32_t* kv_start) {
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
  // absolute key positions: stored row t of the (host-shifted) store is key lo0 + t, chunk token j is key Tabs + j. This batch
  // row's start, clamped to [0, Tabs + S]; lower bound of chunk position s: lb(s) = max(start, Tabs + s + 1 - W)
  const uint32_t Tabs = lo0 + a.T;
  const int32_t ks_raw = *reinterpret_cast<const __attribute__((address_space(4))) int32_t*>(reinterpret_cast<uintptr_t>(kv_start) + 4u * (uintptr_t)b);
  const uint32_t kstart = ks_raw < 0 ? 0u : ((uint32_t)ks_raw < Tabs + a.S ? (uint32_t)ks_raw : Tabs + a.S);
  auto lb = [&](const uint32_t s) -> uint32_t {
    const uint32_t wl = (W && Tabs + s + 1u > W) ? Tabs + s + 1u - W : 0u;
    return wl > kstart ? wl : kstart;
  };

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
  // the first stored / chunk tile inside the window of the workgroup's first chunk position (every later row's window starts
  // later): the tiles before them are not walked
  const uint32_t s_min = (qb * kExtQB) / a.nq;
  const uint32_t lb_min = lb(s_min);  // the smallest lower bound of the workgroup's rows (lb is non-decreasing in s); >= lo0
  const uint32_t t_vis = lb_min > lo0 ? lb_min - lo0 : 0u;  // first stored row the workgroup's first chunk position sees
  uint32_t i_beg = t_vis > st0 ? (t_vis - st0) / kExtTC : 0u;
  i_beg = i_beg < n_st ? i_beg : n_st;
  const uint32_t j_vis = lb_min > Tabs ? lb_min - Tabs : 0u;  // first chunk token row s_min sees
  const uint32_t row_lb = lb(s_row);  // this lane's own lower bound
  const uint32_t j_beg = j_vis / kExtTC < n_new ? j_vis / kExtTC : n_new;
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
      if (t < st1 && lo0 + t >= kstart) {  // rows before this batch row's start are never read: zero codes
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
      const bool live = t < st1 && lo0 + t >= kstart;  // scales past the split's tokens or before the row's start are never read
      skr = live ? a.k_scale[t] : 0.f;
      svr = live ? a.v_scale[t] : 0.f;
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
      if (j < a.S && Tabs + j >= kstart) {  // chunk tokens before this batch row's start are never read: zeros
        kw = *reinterpret_cast<const u32x4*>(knp + (int64_t)j * a.kn_ss + 8u * c);
        vw = *reinterpret_cast<const u32x4*>(vnp + (int64_t)j * a.vn_ss + 8u * c);
      }
      *reinterpret_cast<u32x4*>(&s_k[o * KLD + c * 8u]) = kw;
      const uint32_t pos = ext_vpos(o);
#pragma unroll
      for (int e = 0; e < 8; ++e) s_vt[(c * 8u + e) * VLD + pos] = (uint16_t)((vw[e >> 1] >> (16 * (e & 1))) & 0xFFFFu);
    }
    if (tid < (uint32_t)kExtTC) {
      const float one = (j0 + tid < a.S && Tabs + j0 + tid >= kstart) ? 1.f : 0.f;
      s_sk[tid] = one;
      s_sv[tid] = one;
    }
  };

  float m = -INFINITY, l = 0.f, svref = 0.f;
  f32x4 acc[DB];
#pragma unroll
  for (int n = 0; n < DB; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

  // loop index it walks stored tiles [i_beg, n_st), then chunk tiles j_beg ... (it - n_st + j_beg)
  const uint32_t ntile = n_st + n_new - j_beg;
  if (i_beg < n_st) load_stored(i_beg);
  for (uint32_t it = i_beg; it < ntile; ++it) {
    const bool is_new = it >= n_st;
    const uint32_t t0 = is_new ? (it - n_st + j_beg) * kExtTC : st0 + it * kExtTC;  // chunk position / stored token of tile row 0
    if (is_new) stage_new(t0);
    else stage_stored();
    __syncthreads();
    if (it + 1u < n_st) load_stored(it + 1u);  // in flight while this tile is reduced
    const uint32_t nvalid = is_new ? 0u : (st1 - t0 < (uint32_t)kExtTC ? st1 - t0 : (uint32_t)kExtTC);
    const uint32_t s_wmin = wrow0 / a.nq;  // first chunk position of the wave's rows
    // the tile lies before the window of every row of the wave
    const bool w_out = (is_new ? Tabs : lo0) + t0 + (uint32_t)kExtTC - 1u < lb(s_wmin);
    if (wave_live && !(is_new && t0 > s_wave) && !w_out) {
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
          const bool ok = is_new ? t0 + o <= s_row && Tabs + t0 + o >= row_lb : o < nvalid && lo0 + t0 + o >= row_lb;
          p[i][r] = ok ? sc[i][r] * s_sk[o] * a.scale_log2 : -INFINITY;
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
    const float sc = l > 0.f ? svref / l : 0.f;  // a row that sees no key (its own position is padding): zeros
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

// extend_attn_merge_k for a left-padded batch: a row for which every split has l = 0 (its own position is padding) writes zeros.
// one wave per query row: out = sum_i e^(m_i - M) acc_i / sum_i e^(m_i - M) l_i over the splits (log2 domain)
template <int HD, int DT>
__global__ __launch_bounds__(256) void extend_attn_merge_padded_k(const ExtendArgs a) {
  constexpr int EPL = HD / 64;  // output elements per lane
  const uint32_t lane = threadIdx.x & 63u, row = blockIdx.x * 4u + (threadIdx.x >> 6), bk = blockIdx.y;
  if (row >= a.M) return;
  const uint32_t b = bk / a.Hkv, hk = bk - b * a.Hkv, s_row = row / a.nq, h_row = row - s_row * a.nq;
  const int64_t mp = (int64_t)a.nqb * kExtQB, base = (int64_t)bk * a.nsplit * mp + row;
  float mmax = -INFINITY;
  for (uint32_t sp = 0; sp < a.nsplit; ++sp) mmax = fmaxf(mmax, a.ws[2 * (base + sp * mp)]);
  float L = 0.f, o[EPL];
#pragma unroll
  for (int k = 0; k < EPL; ++k) o[k] = 0.f;
  for (uint32_t sp = 0; sp < a.nsplit; ++sp) {
    const int64_t pr = base + sp * mp;
    const float e = mmax == -INFINITY ? 0.f : exp2f(a.ws[2 * pr] - mmax);  // no split saw a key: weights 0
    L += a.ws[2 * pr + 1] * e;
    const float* ap = a.ws + a.acc_off + pr * HD + EPL * lane;
#pragma unroll
    for (int k = 0; k < EPL; ++k) o[k] += e * ap[k];
  }
  const float inv = L > 0.f ? 1.f / L : 0.f;
  uint16_t* op = reinterpret_cast<uint16_t*>(a.out) + (int64_t)b * a.o_sb + (int64_t)(hk * a.nq + h_row) * a.o_sh +
                 (int64_t)s_row * a.o_ss + EPL * lane;
  if constexpr (EPL == 2) *reinterpret_cast<uint32_t*>(op) = Elem<DT>::pack2(o[0] * inv, o[1] * inv);
  else *op = (uint16_t)(Elem<DT>::pack2(o[0] * inv, 0.f) & 0xFFFFu);
}

// Launch shape: query blocks x splits x (batch row, kv head). Splits over the stored tokens until the launch has about
// kExtTargetWG workgroups, at least two tiles per split. *ns_bound: the split count before rounding to whole tiles per split
// (>= nsplit, monotone in T: what the workspace is sized for).
static bool extend_plan(const kvq_extend_dims_t* d, uint32_t* nqb, uint32_t* nsplit, uint32_t* tps, uint32_t* ns_bound) {
  const int64_t nq = d->Hq / d->Hkv, M = d->S * nq;
  const int64_t qbn = (M + kExtQB - 1) / kExtQB;
  const int64_t ntiles = (d->T + kExtTC - 1) / kExtTC;
  const int64_t base = qbn * d->B * d->Hkv;
  int64_t ns = 1;
  if (ntiles > 0) {
    ns = (kExtTargetWG + base - 1) / base;
    const int64_t by_tiles = (ntiles + 1) / 2;
    if (ns > by_tiles) ns = by_tiles;
    if (ns > kExtMaxSplit) ns = kExtMaxSplit;
    if (ns < 1) ns = 1;
  }
  const int64_t per = ntiles > 0 ? (ntiles + ns - 1) / ns : 0;
  *nqb = (uint32_t)qbn;
  *tps = (uint32_t)per;
  *nsplit = ntiles > 0 ? (uint32_t)((ntiles + per - 1) / per) : 1u;
  *ns_bound = (uint32_t)ns;
  return true;
}

static const char* extend_dims_error(const kvq_extend_dims_t* d) {
  if (d->B <= 0 || d->Hq <= 0 || d->Hkv <= 0 || d->T < 0 || d->S <= 0 || d->D <= 0) return "B, Hq, Hkv, S, D must be positive and T >= 0";
  if (d->Hq % d->Hkv != 0 || d->Hq / d->Hkv > 16) return "need Hq % Hkv == 0 and Hq / Hkv <= 16";
  if (d->B * d->Hkv >= 65536) return "B * Hkv must stay below 65536";
  if (d->T >= (int64_t(1) << 31) - kExtTC || d->S >= (int64_t(1) << 24)) return "T must stay below 2^31 and S below 2^24";
  if (d->D != 64 && d->D != 128) return "head_dim must be 64 or 128";
  return nullptr;
}

static int64_t extend_workspace_floats(const kvq_extend_dims_t* d) {
  uint32_t nqb, ns, tps, nsb;
  extend_plan(d, &nqb, &ns, &tps, &nsb);
  if (nsb <= 1u) return 0;
  const int64_t rows = d->B * d->Hkv * (int64_t)nsb * nqb * kExtQB;
  return (rows * 2 + 3) / 4 * 4 + rows * d->D;
}

template <int KBITS, int VBITS>
static void launch_extend(const ExtendArgs& a, const int D, const int dtype, hipStream_t st, const uint32_t W, const uint32_t neg,
                          const uint32_t lo0 = 0u, const int32_t* kv_start = nullptr) {
  const dim3 grid(a.nqb, a.nsplit, a.B * a.Hkv);
  if (kv_start) {  // a left-padded batch, with or without a window
    if (D == 128) {
      if (dtype == KVQ_F16) KVQ_LAUNCH((extend_attn_padded_k<KBITS, VBITS, 128, KVQ_F16>), grid, dim3(256), 0, st, a, W, lo0, kv_start);
      else KVQ_LAUNCH((extend_attn_padded_k<KBITS, VBITS, 128, KVQ_BF16>), grid, dim3(256), 0, st, a, W, lo0, kv_start);
    } else {
      if (dtype == KVQ_F16) KVQ_LAUNCH((extend_attn_padded_k<KBITS, VBITS, 64, KVQ_F16>), grid, dim3(256), 0, st, a, W, lo0, kv_start);
      else KVQ_LAUNCH((extend_attn_padded_k<KBITS, VBITS, 64, KVQ_BF16>), grid, dim3(256), 0, st, a, W, lo0, kv_start);
    }
    return;
  }
  if (W) {  // a window that cuts something
    if (D == 128) {
      if (dtype == KVQ_F16) KVQ_LAUNCH((extend_attn_window_k<KBITS, VBITS, 128, KVQ_F16>), grid, dim3(256), 0, st, a, W, neg);
      else KVQ_LAUNCH((extend_attn_window_k<KBITS, VBITS, 128, KVQ_BF16>), grid, dim3(256), 0, st, a, W, neg);
    } else {
      if (dtype == KVQ_F16) KVQ_LAUNCH((extend_attn_window_k<KBITS, VBITS, 64, KVQ_F16>), grid, dim3(256), 0, st, a, W, neg);
      else KVQ_LAUNCH((extend_attn_window_k<KBITS, VBITS, 64, KVQ_BF16>), grid, dim3(256), 0, st, a, W, neg);
    }
    return;
  }
  if (D == 128) {
    if (dtype == KVQ_F16) KVQ_LAUNCH((extend_attn_k<KBITS, VBITS, 128, KVQ_F16>), grid, dim3(256), 0, st, a);
    else KVQ_LAUNCH((extend_attn_k<KBITS, VBITS, 128, KVQ_BF16>), grid, dim3(256), 0, st, a);
  } else {
    if (dtype == KVQ_F16) KVQ_LAUNCH((extend_attn_k<KBITS, VBITS, 64, KVQ_F16>), grid, dim3(256), 0, st, a);
    else KVQ_LAUNCH((extend_attn_k<KBITS, VBITS, 64, KVQ_BF16>), grid, dim3(256), 0, st, a);
  }
}

// shared body of kvq_extend_attn / kvq_extend_attn_window; W = 0: no window (today's kernels and arguments)
static int extend_attn_impl(const char* name, const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const uint8_t* k_store,
                            const kvq_strides_t* k_st, const float* k_scales, int k_bits, const uint8_t* v_store,
                            const kvq_strides_t* v_st, const float* v_scales, int v_bits, const void* k_new, int64_t kn_sb,
                            int64_t kn_sh, int64_t kn_ss, const void* v_new, int64_t vn_sb, int64_t vn_sh, int64_t vn_ss, void* out,
                            int64_t o_sb, int64_t o_sh, int64_t o_ss, int dtype, float sm_scale, int64_t window, float* workspace,
                            int64_t workspace_floats, const kvq_extend_dims_t* d_in, void* stream, const int32_t* kv_start = nullptr);

}  // namespace kvq

extern "C" {

int64_t kvq_extend_attn_workspace(const kvq_extend_dims_t* d) {
  if (!d || kvq::extend_dims_error(d)) return -1;
  return kvq::extend_workspace_floats(d);
}

int kvq_extend_attn(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const uint8_t* k_store, const kvq_strides_t* k_st,
                    const float* k_scales, int k_bits, const uint8_t* v_store, const kvq_strides_t* v_st, const float* v_scales,
                    int v_bits, const void* k_new, int64_t kn_sb, int64_t kn_sh, int64_t kn_ss, const void* v_new, int64_t vn_sb,
                    int64_t vn_sh, int64_t vn_ss, void* out, int64_t o_sb, int64_t o_sh, int64_t o_ss, int dtype, float sm_scale,
                    float* workspace, int64_t workspace_floats, const kvq_extend_dims_t* d, void* stream) {
  return kvq::extend_attn_impl("kvq_extend_attn", q, q_sb, q_sh, q_ss, k_store, k_st, k_scales, k_bits, v_store, v_st, v_scales, v_bits,
                               k_new, kn_sb, kn_sh, kn_ss, v_new, vn_sb, vn_sh, vn_ss, out, o_sb, o_sh, o_ss, dtype, sm_scale, 0,
                               workspace, workspace_floats, d, stream);
}

int kvq_extend_attn_window(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const uint8_t* k_store, const kvq_strides_t* k_st,
                           const float* k_scales, int k_bits, const uint8_t* v_store, const kvq_strides_t* v_st, const float* v_scales,
                           int v_bits, const void* k_new, int64_t kn_sb, int64_t kn_sh, int64_t kn_ss, const void* v_new, int64_t vn_sb,
                           int64_t vn_sh, int64_t vn_ss, void* out, int64_t o_sb, int64_t o_sh, int64_t o_ss, int dtype, float sm_scale,
                           int64_t window, float* workspace, int64_t workspace_floats, const kvq_extend_dims_t* d, void* stream) {
  return kvq::extend_attn_impl("kvq_extend_attn_window", q, q_sb, q_sh, q_ss, k_store, k_st, k_scales, k_bits, v_store, v_st, v_scales,
                               v_bits, k_new, kn_sb, kn_sh, kn_ss, v_new, vn_sb, vn_sh, vn_ss, out, o_sb, o_sh, o_ss, dtype, sm_scale,
                               window, workspace, workspace_floats, d, stream);
}

int kvq_extend_attn_padded(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const uint8_t* k_store, const kvq_strides_t* k_st,
                           const float* k_scales, int k_bits, const uint8_t* v_store, const kvq_strides_t* v_st, const float* v_scales,
                           int v_bits, const void* k_new, int64_t kn_sb, int64_t kn_sh, int64_t kn_ss, const void* v_new, int64_t vn_sb,
                           int64_t vn_sh, int64_t vn_ss, void* out, int64_t o_sb, int64_t o_sh, int64_t o_ss, int dtype, float sm_scale,
                           int64_t window, const int32_t* kv_start, float* workspace, int64_t workspace_floats,
                           const kvq_extend_dims_t* d, void* stream) {
  return kvq::extend_attn_impl(kv_start ? "kvq_extend_attn_padded" : "kvq_extend_attn_window", q, q_sb, q_sh, q_ss, k_store, k_st,
                               k_scales, k_bits, v_store, v_st, v_scales, v_bits, k_new, kn_sb, kn_sh, kn_ss, v_new, vn_sb, vn_sh, vn_ss,
                               out, o_sb, o_sh, o_ss, dtype, sm_scale, window, workspace, workspace_floats, d, stream, kv_start);
}

}  // extern "C"

namespace kvq {

static int extend_attn_impl(const char* name, const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const uint8_t* k_store,
                            const kvq_strides_t* k_st, const float* k_scales, int k_bits, const uint8_t* v_store,
                            const kvq_strides_t* v_st, const float* v_scales, int v_bits, const void* k_new, int64_t kn_sb,
                            int64_t kn_sh, int64_t kn_ss, const void* v_new, int64_t vn_sb, int64_t vn_sh, int64_t vn_ss, void* out,
                            int64_t o_sb, int64_t o_sh, int64_t o_ss, int dtype, float sm_scale, int64_t window, float* workspace,
                            int64_t workspace_floats, const kvq_extend_dims_t* d_in, void* stream, const int32_t* kv_start) {
  if (window < 0) {
    set_error("%s: window %lld must be >= 0 (0 = none)", name, (long long)window);
    return KVQ_E_DIMS;
  }
  const kvq_extend_dims_t* d = d_in;
  if (!d || !q || !out || !k_new || !v_new) {
    set_error("%s: NULL q / k_new / v_new / out / dims", name);
    return KVQ_E_NULL;
  }
  if (const char* why = extend_dims_error(d)) {
    set_error("%s: bad dims B=%lld Hq=%lld Hkv=%lld T=%lld S=%lld D=%lld: %s", name, (long long)d->B, (long long)d->Hq,
              (long long)d->Hkv, (long long)d->T, (long long)d->S, (long long)d->D, why);
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
  if (d->T > 0 && (!k_store || !v_store || !k_scales || !v_scales || !k_st || !v_st)) {
    set_error("%s: NULL store / scales / strides", name);
    return KVQ_E_NULL;
  }
  const int64_t need = extend_workspace_floats(d);
  if (need > 0 && (!workspace || workspace_floats < need)) {
    set_error("%s: workspace of %lld floats, %lld needed", name, (long long)(workspace ? workspace_floats : 0), (long long)need);
    return workspace ? KVQ_E_DIMS : KVQ_E_NULL;
  }
  if (need > 0 && !aligned(workspace, 16)) {
    set_error("%s: workspace must be 16-byte aligned", name);
    return KVQ_E_DIMS;
  }
  const int kal = k_bits == 8 ? 16 : 8, val = v_bits == 8 ? 16 : 8;
  if (d->T > 0 && (!aligned(k_store, kal) || k_st->b % kal || k_st->h % kal || k_st->t % kal || !aligned(v_store, val) ||
                   v_st->b % val || v_st->h % val || v_st->t % val)) {
    set_error("%s: store rows must be %d / %d byte aligned", name, kal, val);
    return KVQ_E_DIMS;
  }
  if (d->T > 0 && (k_st->t < d->D * k_bits / 8 || v_st->t < d->D * v_bits / 8)) {
    set_error("%s: store token stride shorter than a row", name);
    return KVQ_E_DIMS;
  }
  const void* bufs[4] = {q, k_new, v_new, out};
  const int64_t strides[12] = {q_sb, q_sh, q_ss, kn_sb, kn_sh, kn_ss, vn_sb, vn_sh, vn_ss, o_sb, o_sh, o_ss};
  for (int i = 0; i < 4; ++i)
    if (!aligned(bufs[i], 16) || strides[3 * i] % 8 || strides[3 * i + 1] % 8 || strides[3 * i + 2] % 8) {
      set_error("%s: q / k_new / v_new / out must be 16-byte aligned with strides that are multiples of 8 elements", name);
      return KVQ_E_DIMS;
    }
  if (const int rcd = check_device(out, name)) return rcd;
  if (kv_start) {
    if (const int rcd = check_device(kv_start, name)) return rcd;
  }

  // A window that cuts something (W < T + S): the stored tokens before lo0 = max(0, T + 1 - W) are seen by no query row and
  // never read; the store starts at lo0 and the kernel masks each row's lower edge. Otherwise today's kernels, unchanged.
  uint32_t W = 0u, neg = 0u, lo0u = 0u;  // lo0u: where the shifted store starts (the padded kernel works in absolute key positions)
  kvq_extend_dims_t dw;
  if (window > 0 && window < d->T + d->S) {
    const int64_t lo0 = d->T + 1 - window > 0 ? d->T + 1 - window : 0;
    dw = *d;
    dw.T = d->T - lo0;
    if (lo0 > 0) {
      k_store += lo0 * k_st->t;
      v_store += lo0 * v_st->t;
      k_scales += lo0;
      v_scales += lo0;
    }
    d = &dw;
    W = (uint32_t)window;
    neg = (uint32_t)(window - 1 - dw.T);
    lo0u = (uint32_t)lo0;
  }

  ExtendArgs a;
  a.q = q; a.q_sb = q_sb; a.q_sh = q_sh; a.q_ss = q_ss;
  a.k = k_store; a.v = v_store;
  if (d->T > 0) {
    a.k_sb = k_st->b; a.k_sh = k_st->h; a.k_st = k_st->t;
    a.v_sb = v_st->b; a.v_sh = v_st->h; a.v_st = v_st->t;
  } else {
    a.k_sb = a.k_sh = a.k_st = a.v_sb = a.v_sh = a.v_st = 0;
  }
  a.k_scale = k_scales; a.v_scale = v_scales;
  a.kn = k_new; a.kn_sb = kn_sb; a.kn_sh = kn_sh; a.kn_ss = kn_ss;
  a.vn = v_new; a.vn_sb = vn_sb; a.vn_sh = vn_sh; a.vn_ss = vn_ss;
  a.out = out; a.o_sb = o_sb; a.o_sh = o_sh; a.o_ss = o_ss;
  a.scale_log2 = sm_scale * 1.4426950408889634f;
  a.B = (uint32_t)d->B; a.Hkv = (uint32_t)d->Hkv; a.nq = (uint32_t)(d->Hq / d->Hkv);
  a.T = (uint32_t)d->T; a.S = (uint32_t)d->S; a.M = (uint32_t)(d->S * (d->Hq / d->Hkv));
  uint32_t nsb;
  extend_plan(d, &a.nqb, &a.nsplit, &a.tps, &nsb);
  a.ws = workspace;
  a.acc_off = ((int64_t)a.B * a.Hkv * a.nsplit * a.nqb * kExtQB * 2 + 3) / 4 * 4;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (k_bits == 8 && v_bits == 8) launch_extend<8, 8>(a, (int)d->D, dtype, st, W, neg, lo0u, kv_start);
  else if (k_bits == 8) launch_extend<8, 4>(a, (int)d->D, dtype, st, W, neg, lo0u, kv_start);
  else if (v_bits == 8) launch_extend<4, 8>(a, (int)d->D, dtype, st, W, neg, lo0u, kv_start);
  else launch_extend<4, 4>(a, (int)d->D, dtype, st, W, neg, lo0u, kv_start);
  int rc = check_launch(name);
  if (rc || a.nsplit == 1u) return rc;
  const dim3 mgrid((a.M + 3u) / 4u, a.B * a.Hkv);
  if (kv_start) {  // rows whose own position is padding: every split has l = 0
    if (d->D == 128) {
      if (dtype == KVQ_F16) KVQ_LAUNCH((extend_attn_merge_padded_k<128, KVQ_F16>), mgrid, dim3(256), 0, st, a);
      else KVQ_LAUNCH((extend_attn_merge_padded_k<128, KVQ_BF16>), mgrid, dim3(256), 0, st, a);
    } else {
      if (dtype == KVQ_F16) KVQ_LAUNCH((extend_attn_merge_padded_k<64, KVQ_F16>), mgrid, dim3(256), 0, st, a);
      else KVQ_LAUNCH((extend_attn_merge_padded_k<64, KVQ_BF16>), mgrid, dim3(256), 0, st, a);
    }
    return check_launch(name);
  }
  if (d->D == 128) {
    if (dtype == KVQ_F16) KVQ_LAUNCH((extend_attn_merge_k<128, KVQ_F16>), mgrid, dim3(256), 0, st, a);
    else KVQ_LAUNCH((extend_attn_merge_k<128, KVQ_BF16>), mgrid, dim3(256), 0, st, a);
  } else {
    if (dtype == KVQ_F16) KVQ_LAUNCH((extend_attn_merge_k<64, KVQ_F16>), mgrid, dim3(256), 0, st, a);
    else KVQ_LAUNCH((extend_attn_merge_k<64, KVQ_BF16>), mgrid, dim3(256), 0, st, a);
  }
  return check_launch(name);
}

}  // namespace kvq

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
// The kernel texts are extend_kernel.inc (plain, sliding-window and left-padded variants) and extend_merge_kernel.inc (plain and
// left-padded), included below once per variant; this file holds what they share, the launch plan and the entry points.
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

// extend_attn_k, extend_attn_window_k and extend_attn_padded_k: one kernel text (extend_kernel.inc), compiled three times
#define KVQ_EXT_VARIANT 0
#include "extend_kernel.inc"
#undef KVQ_EXT_VARIANT
#define KVQ_EXT_VARIANT 1
#include "extend_kernel.inc"
#undef KVQ_EXT_VARIANT
#define KVQ_EXT_VARIANT 2
#include "extend_kernel.inc"
#undef KVQ_EXT_VARIANT

// extend_attn_merge_k and extend_attn_merge_padded_k: one kernel text (extend_merge_kernel.inc), compiled twice
#define KVQ_EXT_MERGE_PADDED 0
#include "extend_merge_kernel.inc"
#undef KVQ_EXT_MERGE_PADDED
#define KVQ_EXT_MERGE_PADDED 1
#include "extend_merge_kernel.inc"
#undef KVQ_EXT_MERGE_PADDED

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

// One launch of KERNEL<TARGS 128 | 64, KVQ_F16 | KVQ_BF16> by head_dim and dtype, 256 threads: the kernel's name, its leading template
// arguments in parentheses ((KBITS, VBITS,) for the extend kernels, () for the merges), then the kernel's arguments. (A macro: a
// function template cannot be passed as a template argument.)
#define KVQ_EXT_TARGS(...) __VA_ARGS__
#define KVQ_EXT_LAUNCH(KERNEL, TARGS, D, DTYPE, GRID, ST, ...)                                                              \
  do {                                                                                                                      \
    if ((D) == 128) {                                                                                                       \
      if ((DTYPE) == KVQ_F16) KVQ_LAUNCH((KERNEL<KVQ_EXT_TARGS TARGS 128, KVQ_F16>), GRID, dim3(256), 0, ST, __VA_ARGS__);  \
      else KVQ_LAUNCH((KERNEL<KVQ_EXT_TARGS TARGS 128, KVQ_BF16>), GRID, dim3(256), 0, ST, __VA_ARGS__);                    \
    } else {                                                                                                                \
      if ((DTYPE) == KVQ_F16) KVQ_LAUNCH((KERNEL<KVQ_EXT_TARGS TARGS 64, KVQ_F16>), GRID, dim3(256), 0, ST, __VA_ARGS__);   \
      else KVQ_LAUNCH((KERNEL<KVQ_EXT_TARGS TARGS 64, KVQ_BF16>), GRID, dim3(256), 0, ST, __VA_ARGS__);                     \
    }                                                                                                                       \
  } while (0)

template <int KBITS, int VBITS>
static void launch_extend(const ExtendArgs& a, const int D, const int dtype, hipStream_t st, const uint32_t W, const uint32_t neg,
                          const uint32_t lo0 = 0u, const int32_t* kv_start = nullptr) {
  const dim3 grid(a.nqb, a.nsplit, a.B * a.Hkv);
  if (kv_start) KVQ_EXT_LAUNCH(extend_attn_padded_k, (KBITS, VBITS,), D, dtype, grid, st, a, W, lo0, kv_start);  // a left-padded batch, with or without a window
  else if (W) KVQ_EXT_LAUNCH(extend_attn_window_k, (KBITS, VBITS,), D, dtype, grid, st, a, W, neg);  // a window that cuts something
  else KVQ_EXT_LAUNCH(extend_attn_k, (KBITS, VBITS,), D, dtype, grid, st, a);
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
  if (kv_start) KVQ_EXT_LAUNCH(extend_attn_merge_padded_k, (), d->D, dtype, mgrid, st, a);  // rows whose own position is padding: every split has l = 0
  else KVQ_EXT_LAUNCH(extend_attn_merge_k, (), d->D, dtype, mgrid, st, a);
  return check_launch(name);
}

#undef KVQ_EXT_LAUNCH
#undef KVQ_EXT_TARGS

}  // namespace kvq

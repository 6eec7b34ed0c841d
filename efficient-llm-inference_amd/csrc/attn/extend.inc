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
// left-padded), included below once per variant; this file holds what they share, the launch plan, the call record (ExtendCall,
// as host.inc's DecodeCall: the entry points fill one, extend_attn_impl takes it) and the entry points.
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
#define KVQ_EXT_VARIANT 3  // extend_attn_mod_k: soft cap / sinks (kvq_extend_attn_ex)
#include "extend_kernel.inc"
#undef KVQ_EXT_VARIANT

// extend_attn_merge_k and extend_attn_merge_padded_k: one kernel text (extend_merge_kernel.inc), compiled twice
#define KVQ_EXT_MERGE_PADDED 0
#include "extend_merge_kernel.inc"
#undef KVQ_EXT_MERGE_PADDED
#define KVQ_EXT_MERGE_PADDED 1
#include "extend_merge_kernel.inc"
#undef KVQ_EXT_MERGE_PADDED
#define KVQ_EXT_MERGE_PADDED 2  // extend_attn_merge_mod_k
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
                          const uint32_t lo0, const int32_t* kv_start, const AttnMod& mod) {
  const dim3 grid(a.nqb, a.nsplit, a.B * a.Hkv);
  if (mod_active(mod)) KVQ_EXT_LAUNCH(extend_attn_mod_k, (KBITS, VBITS,), D, dtype, grid, st, a, W, lo0, kv_start, mod);  // a soft cap or sinks
  else if (kv_start) KVQ_EXT_LAUNCH(extend_attn_padded_k, (KBITS, VBITS,), D, dtype, grid, st, a, W, lo0, kv_start);  // a left-padded batch, with or without a window
  else if (W) KVQ_EXT_LAUNCH(extend_attn_window_k, (KBITS, VBITS,), D, dtype, grid, st, a, W, neg);  // a window that cuts something
  else KVQ_EXT_LAUNCH(extend_attn_k, (KBITS, VBITS,), D, dtype, grid, st, a);
}

// One extend call, whichever entry point it came through (the fields of host.inc's DecodeCall that extend has).
struct ExtendCall {
  const char* name;  // the entry point, for messages
  Rows q, k_new, v_new;
  OutRows out;
  StoreRef k, v;
  int dtype;
  float sm_scale;
  float* workspace;
  int64_t workspace_floats;
  const kvq_extend_dims_t* d;
  void* stream;
  int64_t window;           // keys a query row sees (0 = all: the unwindowed kernels and arguments)
  const int32_t* kv_start;  // device [B]: a left-padded batch
  float softcap;            // kvq_extend_attn_ex only: soft cap of the scores (0 = none)
  const float* sinks;       // kvq_extend_attn_ex only: device [Hq] sink logits (NULL = none)
};

// every extend entry point ends here
static int extend_attn_impl(const ExtendCall& c) {
  const char* name = c.name;
  const int64_t window = c.window;
  if (window < 0) {
    set_error("%s: window %lld must be >= 0 (0 = none)", name, (long long)window);
    return KVQ_E_DIMS;
  }
  const kvq_extend_dims_t* d = c.d;
  if (!d || !c.q.p || !c.out.p || !c.k_new.p || !c.v_new.p) {
    set_error("%s: NULL q / k_new / v_new / out / dims", name);
    return KVQ_E_NULL;
  }
  if (const char* why = extend_dims_error(d)) {
    set_error("%s: bad dims B=%lld Hq=%lld Hkv=%lld T=%lld S=%lld D=%lld: %s", name, (long long)d->B, (long long)d->Hq,
              (long long)d->Hkv, (long long)d->T, (long long)d->S, (long long)d->D, why);
    return KVQ_E_DIMS;
  }
  if (const int rc = check_dtype(name, c.dtype)) return rc;
  if (const int rc = check_bits(name, c.k.bits, c.v.bits)) return rc;
  if (d->T > 0 && (!c.k.p || !c.v.p || !c.k.scales || !c.v.scales || !c.k.st || !c.v.st)) {
    set_error("%s: NULL store / scales / strides", name);
    return KVQ_E_NULL;
  }
  const int64_t need = extend_workspace_floats(d);
  if (need > 0 && (!c.workspace || c.workspace_floats < need)) {
    set_error("%s: workspace of %lld floats, %lld needed", name, (long long)(c.workspace ? c.workspace_floats : 0), (long long)need);
    return c.workspace ? KVQ_E_DIMS : KVQ_E_NULL;
  }
  if (need > 0 && !aligned(c.workspace, 16)) {
    set_error("%s: workspace must be 16-byte aligned", name);
    return KVQ_E_DIMS;
  }
  if (d->T > 0) {
    if (const int rc = check_store_rows(name, c.k, c.v)) return rc;
  }
  if (d->T > 0 && (c.k.st->t < d->D * c.k.bits / 8 || c.v.st->t < d->D * c.v.bits / 8)) {
    set_error("%s: store token stride shorter than a row", name);
    return KVQ_E_DIMS;
  }
  const Rows in[4] = {c.q, c.k_new, c.v_new, {c.out.p, c.out.sb, c.out.sh, c.out.ss}};
  for (const Rows& r : in)
    if (!aligned(r.p, 16) || r.sb % 8 || r.sh % 8 || r.ss % 8) {
      set_error("%s: q / k_new / v_new / out must be 16-byte aligned with strides that are multiples of 8 elements", name);
      return KVQ_E_DIMS;
    }
  if (const int rcd = check_device(c.out.p, name)) return rcd;
  if (c.kv_start) {
    if (const int rcd = check_device(c.kv_start, name)) return rcd;
  }
  AttnMod mod;
  if (const int rc = attn_mod(name, c.softcap, c.sinks, &mod)) return rc;

  // A window that cuts something (W < T + S): the stored tokens before lo0 = max(0, T + 1 - W) are seen by no query row and
  // never read; the store starts at lo0 and the kernel masks each row's lower edge. Otherwise today's kernels, unchanged.
  uint32_t W = 0u, neg = 0u, lo0u = 0u;  // lo0u: where the shifted store starts (the padded kernel works in absolute key positions)
  StoreRef k = c.k, v = c.v;
  kvq_extend_dims_t dw;
  if (window > 0 && window < d->T + d->S) {
    const int64_t lo0 = d->T + 1 - window > 0 ? d->T + 1 - window : 0;
    dw = *d;
    dw.T = d->T - lo0;
    if (lo0 > 0) {
      k = from_row(c.k, lo0);
      v = from_row(c.v, lo0);
    }
    d = &dw;
    W = (uint32_t)window;
    neg = (uint32_t)(window - 1 - dw.T);
    lo0u = (uint32_t)lo0;
  }

  ExtendArgs a;
  a.q = c.q.p; a.q_sb = c.q.sb; a.q_sh = c.q.sh; a.q_ss = c.q.ss;
  a.k = k.p; a.v = v.p;
  if (d->T > 0) {
    a.k_sb = k.st->b; a.k_sh = k.st->h; a.k_st = k.st->t;
    a.v_sb = v.st->b; a.v_sh = v.st->h; a.v_st = v.st->t;
  } else {
    a.k_sb = a.k_sh = a.k_st = a.v_sb = a.v_sh = a.v_st = 0;
  }
  a.k_scale = k.scales; a.v_scale = v.scales;
  a.kn = c.k_new.p; a.kn_sb = c.k_new.sb; a.kn_sh = c.k_new.sh; a.kn_ss = c.k_new.ss;
  a.vn = c.v_new.p; a.vn_sb = c.v_new.sb; a.vn_sh = c.v_new.sh; a.vn_ss = c.v_new.ss;
  a.out = c.out.p; a.o_sb = c.out.sb; a.o_sh = c.out.sh; a.o_ss = c.out.ss;
  a.scale_log2 = c.sm_scale * 1.4426950408889634f;
  a.B = (uint32_t)d->B; a.Hkv = (uint32_t)d->Hkv; a.nq = (uint32_t)(d->Hq / d->Hkv);
  a.T = (uint32_t)d->T; a.S = (uint32_t)d->S; a.M = (uint32_t)(d->S * (d->Hq / d->Hkv));
  uint32_t nsb;
  extend_plan(d, &a.nqb, &a.nsplit, &a.tps, &nsb);
  a.ws = c.workspace;
  a.acc_off = ((int64_t)a.B * a.Hkv * a.nsplit * a.nqb * kExtQB * 2 + 3) / 4 * 4;
  hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
  const int D = (int)d->D;
  with_bits(k.bits, v.bits, [&](auto kb, auto vb) {
    launch_extend<decltype(kb)::value, decltype(vb)::value>(a, D, c.dtype, st, W, neg, lo0u, c.kv_start, mod);
  });
  int rc = check_launch(name);
  if (rc || a.nsplit == 1u) return rc;
  const dim3 mgrid((a.M + 3u) / 4u, a.B * a.Hkv);
  if (mod_active(mod)) KVQ_EXT_LAUNCH(extend_attn_merge_mod_k, (), D, c.dtype, mgrid, st, a, mod);
  else if (c.kv_start) KVQ_EXT_LAUNCH(extend_attn_merge_padded_k, (), D, c.dtype, mgrid, st, a);  // rows whose own position is padding: every split has l = 0
  else KVQ_EXT_LAUNCH(extend_attn_merge_k, (), D, c.dtype, mgrid, st, a);
  return check_launch(name);
}

#undef KVQ_EXT_LAUNCH
#undef KVQ_EXT_TARGS

}  // namespace kvq

// The shared fields of the three entry points, from their like-named parameters (include/kvq_hip.h); window and kv_start are set
// by the entry points that have them.
#define KVQ_EXTEND_CALL(NAME)                                                                                                \
  kvq::ExtendCall c = {};                                                                                                    \
  c.name = NAME;                                                                                                             \
  c.q = {q, q_sb, q_sh, q_ss}; c.k_new = {k_new, kn_sb, kn_sh, kn_ss}; c.v_new = {v_new, vn_sb, vn_sh, vn_ss};               \
  c.out = {out, o_sb, o_sh, o_ss}; c.k = {k_store, k_st, k_scales, k_bits}; c.v = {v_store, v_st, v_scales, v_bits};         \
  c.dtype = dtype; c.sm_scale = sm_scale; c.workspace = workspace; c.workspace_floats = workspace_floats; c.d = d; c.stream = stream

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
  KVQ_EXTEND_CALL("kvq_extend_attn");
  return kvq::extend_attn_impl(c);
}

int kvq_extend_attn_window(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const uint8_t* k_store, const kvq_strides_t* k_st,
                           const float* k_scales, int k_bits, const uint8_t* v_store, const kvq_strides_t* v_st, const float* v_scales,
                           int v_bits, const void* k_new, int64_t kn_sb, int64_t kn_sh, int64_t kn_ss, const void* v_new, int64_t vn_sb,
                           int64_t vn_sh, int64_t vn_ss, void* out, int64_t o_sb, int64_t o_sh, int64_t o_ss, int dtype, float sm_scale,
                           int64_t window, float* workspace, int64_t workspace_floats, const kvq_extend_dims_t* d, void* stream) {
  KVQ_EXTEND_CALL("kvq_extend_attn_window");
  c.window = window;
  return kvq::extend_attn_impl(c);
}

int kvq_extend_attn_padded(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const uint8_t* k_store, const kvq_strides_t* k_st,
                           const float* k_scales, int k_bits, const uint8_t* v_store, const kvq_strides_t* v_st, const float* v_scales,
                           int v_bits, const void* k_new, int64_t kn_sb, int64_t kn_sh, int64_t kn_ss, const void* v_new, int64_t vn_sb,
                           int64_t vn_sh, int64_t vn_ss, void* out, int64_t o_sb, int64_t o_sh, int64_t o_ss, int dtype, float sm_scale,
                           int64_t window, const int32_t* kv_start, float* workspace, int64_t workspace_floats,
                           const kvq_extend_dims_t* d, void* stream) {
  KVQ_EXTEND_CALL(kv_start ? "kvq_extend_attn_padded" : "kvq_extend_attn_window");
  c.window = window;
  c.kv_start = kv_start;
  return kvq::extend_attn_impl(c);
}

// kvq_extend_attn_padded with its window and kv_start in an options record, plus the two score modifiers. Both off: the padded call.
int kvq_extend_attn_ex(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const uint8_t* k_store, const kvq_strides_t* k_st,
                       const float* k_scales, int k_bits, const uint8_t* v_store, const kvq_strides_t* v_st, const float* v_scales,
                       int v_bits, const void* k_new, int64_t kn_sb, int64_t kn_sh, int64_t kn_ss, const void* v_new, int64_t vn_sb,
                       int64_t vn_sh, int64_t vn_ss, void* out, int64_t o_sb, int64_t o_sh, int64_t o_ss, int dtype, float sm_scale,
                       const kvq_attn_opts_t* opts, float* workspace, int64_t workspace_floats, const kvq_extend_dims_t* d,
                       void* stream) {
  if (!opts) {
    kvq::set_error("kvq_extend_attn_ex: NULL opts");
    return KVQ_E_NULL;
  }
  const bool mods = opts->softcap != 0.0f || opts->sinks;
  KVQ_EXTEND_CALL(mods ? "kvq_extend_attn_ex" : opts->kv_start ? "kvq_extend_attn_padded" : "kvq_extend_attn_window");
  c.window = opts->window;
  c.kv_start = opts->kv_start;
  c.softcap = opts->softcap;
  c.sinks = opts->sinks;
  return kvq::extend_attn_impl(c);
}

#undef KVQ_EXTEND_CALL

}  // extern "C"

// kvq_common.h — shared device helpers for the gfx950 KV quantize/dequantize/eviction kernels.
// CDNA4 only: wave64, 16-byte vector memory ops, no portability layer.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/kvq_hip.h"

namespace kvq {

typedef _Float16 f16;
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef f16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int kBlock = 256;  // 4 waves of 64
constexpr int kWave = 64;

struct Strides {
  int64_t g, b, h, t;
};
static inline Strides to_strides(const kvq_strides_t* s) { return Strides{s->g, s->b, s->h, s->t}; }

// Up to KVQ_PTRS_PER_LAUNCH group base pointers travel by value in the kernarg segment, so a
// legacy tuple of separately allocated [B,H,T,D] tensors needs no host->device table copy.
constexpr int kPtrsPerLaunch = 128;
struct PtrTable {
  const void* p[kPtrsPerLaunch];
};

// ------------------------------------------------------------------ error reporting (host)
void set_error(const char* fmt, ...);
int check_launch(const char* what);
int check_device(const void* p, const char* name);  // 0, or KVQ_E_DEVICE when `p` lives on another device than the thread's current one

// kvq_time_next_launch: HIP events the NEXT kernel launch of the calling thread binds to its own dispatch
// (hipExtLaunchKernelGGL start / stop timestamps): the kernel's duration without queue gaps. Taken (and cleared) by
// the first launch that follows, whichever entry point makes it; {nullptr, nullptr} = plain launch.
struct TimingEvents {
  hipEvent_t start, stop;
};
TimingEvents take_timing_events();

// kvq_kernel_log: every launch notes its kernel's host stub; the log resolves the stubs to the names a profiler
// prints (hipKernelNameRefByPtr + demangling), so a benchmark labels its roofline with the kernel that actually ran.
void note_launch(const void* host_stub);

// The one way this library launches a kernel: `kernel` is a __global__ function's host stub — named, or a pointer chosen at
// run time among template instantiations of one signature (attn/host.inc).
// The arguments convert to the kernel's own parameter types at the call, as in a direct call of the kernel.
template <class... Params>
static inline void launch(void (*kernel)(Params...), const dim3 grid, const dim3 block, const size_t lds, hipStream_t st,
                          const std::common_type_t<Params>... args) {
  note_launch(reinterpret_cast<const void*>(kernel));
  const TimingEvents ev = take_timing_events();
  if (ev.start || ev.stop) hipExtLaunchKernelGGL(kernel, grid, block, lds, st, ev.start, ev.stop, 0, args...);
  else hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
}
#define KVQ_LAUNCH(KERNEL, GRID, BLOCK, LDS, ST, ...) ::kvq::launch(KERNEL, GRID, BLOCK, LDS, ST, __VA_ARGS__)

// Process-global test knobs (kvq_set_tunable). Each routes a call to shipped code it would not take by size or shape, so
// that the tests reach every kernel the library holds; the defaults are what ships.
struct Tunables {
  int64_t quant_force_two_pass;  // 1 = generic two-pass quantise for every shape
  int64_t quant_direct_stores;   // 1 = skip the LDS-staged 16 B stores of the 256-thread fused kernel
  int64_t quant_block;           // general fused quantise kernel: 64 (default, one wave per tile); anything else = 256 threads (measured: 241 / 270 us)
  int64_t quant_wide;            // 1 (default) = single-pass 1024-thread register tile for batched slices of 16384 < B*H*D <= 131072 elements; 0 = split phases / swept tile
  int64_t quant_tile;            // 1 (default) = compile-time-geometry one-wave tile kernel where the shape has one; 0 = general kernels
  int64_t quant_few_tokens;      // abs-max phase of a slice of at most this many tokens (a sharded decode append: 1): one workgroup per (group, token) and a plain store instead of the tile walk's atomics on one word; 0 = never
  int64_t gather_rows;           // token gather: 1 (default) = 4 KiB work items, one 16-byte piece per thread (gather_rows_k); 0 = the grid-stride kernel (same bytes)
  int64_t pool_wave;             // chunk mean-pool: one wave per output row when the shape allows (1, default) or the per-lane-group walk (0)
  int64_t store_pool_fast;       // kvq_store_chunk_pool: 1 (default) = 16-byte pieces in registers where the layout allows (store_pool_fast_k); 0 = the generic kernel (same bits)
  int64_t attn_force_valu;       // 1 = decode attention never takes an MFMA kernel
  int64_t attn_stream_tpw;       // ring kernel: 64-token tiles per wave; 0 = by size (only when tiles exceed wave slots), -1 = never
  int64_t attn_lds;              // ring kernel (LDS-staged streaming): -1 = by shape (default), 0 = never
  int64_t attn_ring_dev;         // kvq_decode_step_dev (device-side token count) on the ring kernel where the host-side call takes it (1, default); 0 = always one-tile splits
  int64_t attn_merge_wave;       // merge of <= 16 splits at head_dim 128: 1 (default) = one wave per head, 0 = the 256-thread workgroup per head (same bits)
  int64_t attn_merge_fast;       // 1 (default) = merge kernel that requests everything up front (<= 256 splits); 0 = the chained decode_attn_merge_k (any number of splits)
  int64_t attn_new_token_parts;  // decode step, new-token slices past 8,192 elements: one workgroup per 8,192 elements, each taking the whole slice's abs-max (1, default); 0 = the generic one-workgroup routine
};
Tunables& tunables();


// ------------------------------------------------------------------ element conversion

template <int DT>
struct Elem;  // storage type + widen/narrow (RN-even, what torch .float()/.to(dtype) do)

template <>
struct Elem<KVQ_F16> {
  typedef f16 type;
  static constexpr int size = 2;
  __device__ static inline float widen(uint16_t bits) {
    f16 h;
    __builtin_memcpy(&h, &bits, 2);
    return (float)h;
  }
  __device__ static inline uint32_t pack2(float a, float b) {
    f16x2 v = {(f16)a, (f16)b};
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return u;
  }
  __device__ static inline float round_trip(float v) { return (float)(f16)v; }
};

template <>
struct Elem<KVQ_BF16> {
  typedef __bf16 type;
  static constexpr int size = 2;
  __device__ static inline float widen(uint16_t bits) { return __uint_as_float((uint32_t)bits << 16); }
  __device__ static inline uint32_t pack2(float a, float b) {
    bf16x2 v = {(__bf16)a, (__bf16)b};
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return u;
  }
  __device__ static inline float round_trip(float v) { return (float)(__bf16)v; }
};

template <>
struct Elem<KVQ_F32> {
  typedef float type;
  static constexpr int size = 4;
  __device__ static inline float round_trip(float v) { return v; }
};

// Load 8 consecutive elements (16-byte aligned for 2-byte types, 32 bytes for f32) as fp32.
template <int DT>
__device__ inline void load8(const void* p, float (&x)[8]) {
  if constexpr (DT == KVQ_F32) {
    const u32x4 a = *reinterpret_cast<const u32x4*>(p);
    const u32x4 b = *(reinterpret_cast<const u32x4*>(p) + 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      x[i] = __uint_as_float(a[i]);
      x[4 + i] = __uint_as_float(b[i]);
    }
  } else {
    const u32x4 a = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      x[2 * i] = Elem<DT>::widen((uint16_t)(a[i] & 0xFFFFu));
      x[2 * i + 1] = Elem<DT>::widen((uint16_t)(a[i] >> 16));
    }
  }
}

// Store 8 fp32 values as 8 consecutive elements of DT (RN-even), 16-byte vector stores.
template <int DT, bool NT>
__device__ inline void store8(void* p, const float (&x)[8]) {
  if constexpr (DT == KVQ_F32) {
    u32x4 a, b;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[i] = __float_as_uint(x[i]);
      b[i] = __float_as_uint(x[4 + i]);
    }
    if constexpr (NT) {
      __builtin_nontemporal_store(a, reinterpret_cast<u32x4*>(p));
      __builtin_nontemporal_store(b, reinterpret_cast<u32x4*>(p) + 1);
    } else {
      *reinterpret_cast<u32x4*>(p) = a;
      *(reinterpret_cast<u32x4*>(p) + 1) = b;
    }
  } else {
    u32x4 a;
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = Elem<DT>::pack2(x[2 * i], x[2 * i + 1]);
    if constexpr (NT) {
      __builtin_nontemporal_store(a, reinterpret_cast<u32x4*>(p));
    } else {
      *reinterpret_cast<u32x4*>(p) = a;
    }
  }
}

// Tile element storage: 2-byte dtypes stay PACKED in registers (4 VGPRs per 8 elements) between
// the abs-max pass and the quantise pass; fp32 keeps 8 floats.
template <int IDT>
struct Vec8 {
  u32x4 w;
  __device__ inline void load(const void* p) { w = *reinterpret_cast<const u32x4*>(p); }
  // read-once stream: non-temporal (keeps the line out of the way of the stores' write-back)
  __device__ inline void load_nt(const void* p) { w = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)); }
  // max |x| as an order-preserving bit pattern: sign-masked halves compared as unsigned ints
  __device__ inline uint32_t absmax_bits() const {
    typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
    u16x2 h[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t a = w[i] & 0x7FFF7FFFu;
      __builtin_memcpy(&h[i], &a, 4);
    }
    const u16x2 m = __builtin_elementwise_max(__builtin_elementwise_max(h[0], h[1]),
                                              __builtin_elementwise_max(h[2], h[3]));  // v_pk_max_u16
    return max((uint32_t)m[0], (uint32_t)m[1]);
  }
  __device__ static inline float bits_to_f32(uint32_t b) { return Elem<IDT>::widen((uint16_t)b); }
  // a NaN's pattern lies above +inf's, so the unsigned max keeps a NaN element and has_nan() reads it off
  static constexpr uint32_t kInfBits = IDT == KVQ_F16 ? 0x7C00u : 0x7F80u;
  __device__ inline bool has_nan() const { return absmax_bits() > kInfBits; }
  __device__ inline float get(int j) const {
    return Elem<IDT>::widen((uint16_t)((j & 1) ? (w[j >> 1] >> 16) : (w[j >> 1] & 0xFFFFu)));
  }
};
template <>
struct Vec8<KVQ_F32> {
  float x[8];
  __device__ inline void load(const void* p) { load8<KVQ_F32>(p, x); }
  __device__ inline void load_nt(const void* p) { load8<KVQ_F32>(p, x); }
  __device__ inline uint32_t absmax_bits() const {
    uint32_t m = 0u;  // on the patterns, as the packed types do: fmaxf would drop a NaN element
#pragma unroll
    for (int j = 0; j < 8; ++j) m = max(m, __float_as_uint(x[j]) & 0x7FFFFFFFu);
    return m;
  }
  __device__ static inline float bits_to_f32(uint32_t b) { return __uint_as_float(b); }
  static constexpr uint32_t kInfBits = 0x7F800000u;
  __device__ inline bool has_nan() const { return absmax_bits() > kInfBits; }
  __device__ inline float get(int j) const { return x[j]; }
};

// scalar element access for the generic (any shape / stride) kernels
template <int DT>
__device__ inline float load1(const void* base, int64_t idx) {
  if constexpr (DT == KVQ_F32) {
    return reinterpret_cast<const float*>(base)[idx];
  } else {
    return Elem<DT>::widen(reinterpret_cast<const uint16_t*>(base)[idx]);
  }
}
template <int DT>
__device__ inline void store1(void* base, int64_t idx, float v) {
  if constexpr (DT == KVQ_F32) {
    reinterpret_cast<float*>(base)[idx] = v;
  } else {
    reinterpret_cast<uint16_t*>(base)[idx] = (uint16_t)(Elem<DT>::pack2(v, 0.0f) & 0xFFFFu);
  }
}

// fp32 product that stays an fp32 product. Without the opaque barrier hipcc folds
// (f16)(a * b) into v_fma_mixlo_f16 a, b, +0.0, and (-0.0) + (+0.0) = +0.0 loses the sign of a
// zero result (q < 0 with a stored fp16 scale of 0): the reference yields -0.0 there.
__device__ inline float mul_exact(float a, float b) {
  float p = a * b;
  asm("" : "+v"(p));
  return p;
}

// ------------------------------------------------------------------ abs-max with the reference's NaN rule
// torch's abs().max() returns NaN when the slice holds one (ops.py:27, :48) where fmaxf drops it. Values with a clear
// sign bit order like their bit patterns taken as unsigned integers, +inf above every finite value and every NaN above
// +inf: the unsigned max of the patterns is the reference's maximum, NaN included.
__device__ inline float max_nonneg(float a, float b) { return __uint_as_float(max(__float_as_uint(a), __float_as_uint(b))); }
// the same rule for values of either sign (an abs-max table the caller owns): once per token, never per element
__device__ inline float max_keep_nan(float a, float b) { return a != a ? a : b != b ? b : fmaxf(a, b); }

// ------------------------------------------------------------------ wave64 reductions

// max over aligned groups of `width` consecutive lanes (width = power of two <= 64) of non-negative values (max_nonneg:
// a NaN in any lane is the result); every lane of a group receives the group's max.
__device__ inline float group_max(float v, int width) {
  if (width > 1) v = max_nonneg(v, __shfl_xor(v, 1));
  if (width > 2) v = max_nonneg(v, __shfl_xor(v, 2));
  if (width > 4) v = max_nonneg(v, __shfl_xor(v, 4));
  if (width > 8) v = max_nonneg(v, __shfl_xor(v, 8));
  if (width > 16) v = max_nonneg(v, __shfl_xor(v, 16));
  if (width > 32) v = max_nonneg(v, __shfl_xor(v, 32));
  return v;
}

__device__ inline float wave_max(float v) { return group_max(v, 64); }

// block-wide max of non-negative floats through LDS (s_red: >= kBlock/kWave floats)
__device__ inline float block_max_nonneg(float v, float* s_red) {
  v = wave_max(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  float r = s_red[0];
#pragma unroll
  for (int i = 1; i < kBlock / kWave; ++i) r = max_nonneg(r, s_red[i]);
  __syncthreads();
  return r;
}

// ------------------------------------------------------------------ the reference's quantiser, one element
template <int BITS>
struct QRange;
template <>
struct QRange<8> {
  static constexpr float qmax = 127.0f, qmin = -127.0f;
};
template <>
struct QRange<4> {
  static constexpr float qmax = 7.0f, qmin = -8.0f;
};

// The reference's scale (ops.py:28, :49): torch's clamp(min=eps) keeps a NaN abs-max where fmaxf would answer eps.
// A slice with a NaN has the scale NaN, one with an inf and no NaN +inf. Compare and select (a NaN quotient compares
// false and stays): no branch around the division, and fmaxf's value for every other quotient.
template <int BITS>
__device__ inline float scale_of(float amax, float eps) {
  const float s = amax / QRange<BITS>::qmax;
  return s < eps ? eps : s;
}

// A NaN quotient (a NaN element; any element under a NaN scale; inf under an inf scale) is code 0, as the reference's
// cast of NaN to int8 stores it; x / inf = 0 too, so every code of a token whose scale is not finite is 0.
template <int BITS>
__device__ inline int quant1(float x, float s32) {
  const float r = rintf(x / s32);  // IEEE fp32 divide + round-half-even, as torch does
  return r != r ? 0 : (int)fminf(fmaxf(r, QRange<BITS>::qmin), QRange<BITS>::qmax);
}

// K and V of ONE new token (a decode step's append, ops.py:323-330): slice w (0 = K, 1 = V) of
// [B,H,1,D] is quantised by ONE workgroup of kBlock threads into slot T of its store. The slices are
// a few KB, so the arithmetic is the reference's own (IEEE divide per element), bit-identical with
// the bulk kernels by construction. Runs as two extra workgroups of the attention merge launch
// (kvq_decode_step) or as its own two-workgroup launch.
struct NewTokenArgs {
  const void* x[2];
  int64_t xs_b[2], xs_h[2];  // elements
  uint8_t* q[2];             // slot T of the store
  int64_t qs_b[2], qs_h[2];  // bytes
  int64_t qs_t[2];           // bytes per token row (device-side slot: kvq_decode_step_dev)
  float* scale[2];           // &scales[T]
  int32_t bits[2];
  uint32_t B, H, D;
  float eps;
  uint32_t nparts;           // > 1: workgroups per slice (quant_new_token_parts, merge.inc: slices past the register path); 0 / 1: one
};

template <int IDT>
__device__ inline void quant_new_token_block(const NewTokenArgs& a, uint32_t w, float* s_red) {
  const uint32_t tid = threadIdx.x;
  const void* x = a.x[w];
  const uint32_t n = a.B * a.H * a.D;
  float m = 0.0f;
  for (uint32_t i = tid; i < n; i += kBlock) {
    const uint32_t d = i % a.D, r = i / a.D;
    m = max_nonneg(m, fabsf(load1<IDT>(x, (int64_t)(r / a.H) * a.xs_b[w] + (int64_t)(r % a.H) * a.xs_h[w] + d)));
  }
  m = block_max_nonneg(m, s_red);
  if (a.bits[w] == 8) {
    const float s32 = scale_of<8>(m, a.eps);
    if (tid == 0) *a.scale[w] = Elem<IDT>::round_trip(s32);
    for (uint32_t i = tid; i < n; i += kBlock) {
      const uint32_t d = i % a.D, r = i / a.D;
      const float v = load1<IDT>(x, (int64_t)(r / a.H) * a.xs_b[w] + (int64_t)(r % a.H) * a.xs_h[w] + d);
      a.q[w][(int64_t)(r / a.H) * a.qs_b[w] + (int64_t)(r % a.H) * a.qs_h[w] + d] = (uint8_t)(int8_t)quant1<8>(v, s32);
    }
  } else {
    const float s32 = scale_of<4>(m, a.eps);
    if (tid == 0) *a.scale[w] = Elem<IDT>::round_trip(s32);
    const uint32_t Dq = (a.D + 1) / 2;
    for (uint32_t i = tid; i < a.B * a.H * Dq; i += kBlock) {
      const uint32_t j = i % Dq, r = i / Dq;
      const int64_t xo = (int64_t)(r / a.H) * a.xs_b[w] + (int64_t)(r % a.H) * a.xs_h[w];
      const int hi = quant1<4>(load1<IDT>(x, xo + 2 * j), s32) + 8;
      const int lo = 2 * j + 1 < a.D ? quant1<4>(load1<IDT>(x, xo + 2 * j + 1), s32) + 8 : 8;
      a.q[w][(int64_t)(r / a.H) * a.qs_b[w] + (int64_t)(r % a.H) * a.qs_h[w] + j] = (uint8_t)(((hi & 0xF) << 4) | (lo & 0xF));
    }
  }
}

// Workgroup id -> work item with `k` consecutive items per XCD: the dispatcher deals workgroups round robin
// over the 8 XCDs (MI355X_MICROARCH: blocks b and b + 8 share one), so with the identity map XCD x sees
// every 8th item; this map gives it runs of k consecutive items (k x the item's bytes contiguous per XCD L2)
// while all XCDs stay inside one window of 8 k items. Any k gives the same results; it measured no faster, and the
// host passes k = 0 (the identity map). Items past the last complete window keep the identity map.
__device__ inline uint32_t xcd_grouped_item(uint32_t wg, uint32_t k, uint32_t total) {
  if (k <= 1u) return wg;
  const uint32_t win = 8u * k;
  const uint32_t base = wg / win * win;
  if (base + win > total) return wg;
  const uint32_t r = wg - base;
  return base + (r & 7u) * k + (r >> 3);
}

static inline int ilog2_exact(int64_t v) {  // log2 if power of two else -1
  if (v <= 0 || (v & (v - 1))) return -1;
  int s = 0;
  while ((int64_t(1) << s) < v) ++s;
  return s;
}

static inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// Every listed stride (or size) is a multiple of n.
template <class... S>
static inline bool multiples_of(int64_t n, S... strides) { return ((strides % n == 0) && ...); }

// f(std::integral_constant<int, DT>{}) for the dtype code of a call (validated: fp16, bf16 or fp32)
template <class F>
static inline void by_dtype(int dtype, F&& f) {
  if (dtype == KVQ_F16) f(std::integral_constant<int, KVQ_F16>{});
  else if (dtype == KVQ_BF16) f(std::integral_constant<int, KVQ_BF16>{});
  else f(std::integral_constant<int, KVQ_F32>{});
}

// f(g0, gn) -> rc for the launch chunks [g0, g0 + gn) of G groups, per_launch at a time; the first non-zero rc is returned
template <class F>
static inline int for_launch_chunks(int64_t G, int64_t per_launch, F&& f) {
  for (int64_t g0 = 0; g0 < G; g0 += per_launch)
    if (const int rc = f(g0, G - g0 < per_launch ? G - g0 : per_launch)) return rc;
  return 0;
}

// ------------------------------------------------------------------ host: group pointers and argument checks

// Base pointer of group g: the caller's table entry, or g group strides into one allocation.
static inline const void* group_ptr(const void* base, const void* const* ptrs, int64_t g, int64_t stride_g_bytes) {
  return ptrs ? ptrs[g] : static_cast<const char*>(base) + g * stride_g_bytes;
}

// Every group pointer of [g0, g0 + gn) is non-null and 16-byte aligned.
static inline bool ptrs_aligned16(const void* base, const void* const* ptrs, int64_t g0, int64_t gn, int64_t stride_g_bytes) {
  for (int64_t g = g0; g < g0 + gn; ++g) {
    const void* p = group_ptr(base, ptrs, g, stride_g_bytes);
    if (!p || !aligned(p, 16)) return false;
  }
  return true;
}

// The pointer table of one launch: groups [g0, g0 + gn), each advanced by extra_bytes. KVQ_E_NULL for a NULL entry.
static inline int fill_ptrs(PtrTable& tbl, const void* base, const void* const* ptrs, int64_t g0, int64_t gn,
                            int64_t stride_g_bytes, int64_t extra_bytes, const char* name) {
  for (int64_t i = 0; i < gn; ++i) {
    const char* p = static_cast<const char*>(group_ptr(base, ptrs, g0 + i, stride_g_bytes));
    if (!p) {
      set_error("%s: in_ptrs[%lld] is NULL", name, (long long)(g0 + i));
      return KVQ_E_NULL;
    }
    tbl.p[i] = p + extra_bytes;
  }
  return 0;
}

// The checks an entry point over G groups of a [B,H,T,D] input starts with, in this order: NULL arguments (`present`:
// the entry point's own required pointers), the output's device, in_base or in_ptrs but not both, no negative dim.
static inline int check_group_call(bool present, const void* in_base, const void* const* in_ptrs, const void* out,
                                   const kvq_dims_t* d, const char* name) {
  if (!present || !d || (!in_base && !in_ptrs)) {
    set_error("%s: NULL argument", name);
    return KVQ_E_NULL;
  }
  if (const int rc = check_device(out, name)) return rc;
  if (in_base && in_ptrs) {
    set_error("%s: pass in_base or in_ptrs, not both", name);
    return KVQ_E_DIMS;
  }
  if (d->G < 0 || d->B < 0 || d->H < 0 || d->T < 0 || d->D < 0) {
    set_error("%s: bad dims: negative dim", name);
    return KVQ_E_DIMS;
  }
  return 0;
}

}  // namespace kvq

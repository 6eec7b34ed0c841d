// kvq_evict.hip — KV eviction kernels for gfx950: sliding-window compaction and chunk-summary
// mean-pooling over [G,B,H,T,D] tensors.
//
// Replaces trim_kv_sliding_window (src/cache/implementations.py:124-140) and
// chunk_summarize_kv (implementations.py:295-346).
//
// Roofline: HBM streams. Window compaction moves 2*esz bytes per kept element. Mean-pool reads
// every old token once (esz*B*H*D*old) plus the kept tail, writes n_chunks + keep rows: ~64:1
// read-dominated at chunk_size 64.
#include "kvq_common.h"

namespace kvq {

// ---------------------------------------------------------------------------- window compaction

struct CopyArgs {
  PtrTable in;  // per-group source base, already advanced to the first kept token
  Strides isb;  // source strides in BYTES
  char* out;    // destination base of this launch's first group
  Strides osb;  // destination strides in BYTES
  uint32_t BH, H;
  uint32_t segs_per_bh;  // 1 when (t,d) is contiguous on both sides, else W (one segment per token)
  int64_t seg_bytes;     // bytes per segment
  uint32_t cps;          // chunks per segment
  uint32_t one_base;     // 1: ONE allocation, group g starts at in.p[0] + g * isb.g (no 128-pointer limit per launch: a paged pool of thousands of blocks is one launch)
};

constexpr int kCopyUnroll = 1;  // one 16-byte vector per thread + non-temporal load/store: the fastest copy recipe
                                // on this chip (profiles/r01e_microbench_calibration.txt: 6.58 TB/s; 5.9 at 4 vectors)
constexpr int64_t kCopyChunk = (int64_t)kBlock * 16 * kCopyUnroll;  // 4 KiB per work item

template <bool VEC>
__global__ __launch_bounds__(kBlock) void copy_rows_k(const CopyArgs a) {
  const uint32_t g = blockIdx.y;
  uint32_t item = blockIdx.x;
  const uint32_t chunk = item % a.cps;
  item /= a.cps;
  const uint32_t seg = item % a.segs_per_bh;
  const uint32_t bh = item / a.segs_per_bh;
  const uint32_t b = bh / a.H, h = bh - b * a.H;
  const char* gsrc = a.one_base ? reinterpret_cast<const char*>(a.in.p[0]) + (int64_t)g * a.isb.g : reinterpret_cast<const char*>(a.in.p[g]);
  const char* src = gsrc + (int64_t)b * a.isb.b + (int64_t)h * a.isb.h + (int64_t)seg * a.isb.t;
  char* dst = a.out + (int64_t)g * a.osb.g + (int64_t)b * a.osb.b + (int64_t)h * a.osb.h + (int64_t)seg * a.osb.t;
  const int64_t c0 = (int64_t)chunk * kCopyChunk;
  if constexpr (VEC) {
    u32x4 v[kCopyUnroll];
#pragma unroll
    for (int u = 0; u < kCopyUnroll; ++u) {
      const int64_t o = c0 + ((int64_t)u * kBlock + threadIdx.x) * 16;
      if (o < a.seg_bytes) v[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src + o));
    }
#pragma unroll
    for (int u = 0; u < kCopyUnroll; ++u) {
      const int64_t o = c0 + ((int64_t)u * kBlock + threadIdx.x) * 16;
      if (o < a.seg_bytes) __builtin_nontemporal_store(v[u], reinterpret_cast<u32x4*>(dst + o));
    }
  } else {  // 2-byte granularity (elem_size is 2 or 4)
    int64_t c1 = c0 + kCopyChunk;
    if (c1 > a.seg_bytes) c1 = a.seg_bytes;
    for (int64_t o = c0 + (int64_t)threadIdx.x * 2; o < c1; o += kBlock * 2)
      *reinterpret_cast<uint16_t*>(dst + o) = *reinterpret_cast<const uint16_t*>(src + o);
  }
}

// ---------------------------------------------------------------------------- token gather

struct GatherArgs {
  PtrTable in;
  Strides isb;  // bytes
  char* out;
  Strides osb;  // bytes
  const int32_t* idx;
  uint32_t H, n_idx;
  uint32_t T;          // source tokens: idx values outside [0, T) never become an address
  uint32_t row_bytes;  // D * elem_size
  uint32_t vecs;       // 16-byte vectors per token row (VEC) or 2-byte units (scalar)
};

// One lane = one 16-byte piece of one output token row; the lanes of a row read one contiguous
// source row (HBM-bound row gather: 2 * elem_size bytes per kept element). The index table is the
// caller's DEVICE memory: an index outside [0, T) (torch's index_select raises there) writes a
// row of zeros instead of reading out of bounds — one compare per row piece.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void gather_tokens_k(const GatherArgs a, uint32_t items_per_g) {
  const uint32_t g = blockIdx.y;
  constexpr uint32_t kUnit = VEC ? 16u : 2u;
  // 64-bit counter: items_per_g may sit within one grid stride of 2^32
  for (uint64_t it = (uint64_t)blockIdx.x * kBlock + threadIdx.x; it < items_per_g; it += (uint64_t)gridDim.x * kBlock) {
    const uint32_t item = (uint32_t)it;
    const uint32_t v = item % a.vecs;
    uint32_t r = item / a.vecs;
    const uint32_t j = r % a.n_idx;
    r /= a.n_idx;
    const uint32_t h = r % a.H, b = r / a.H;
    const int64_t t = a.idx[j];
    if ((uint64_t)t >= (uint64_t)a.T) {  // also catches negative indices
      char* bad = a.out + (int64_t)g * a.osb.g + (int64_t)b * a.osb.b + (int64_t)h * a.osb.h + (int64_t)j * a.osb.t +
                  (int64_t)v * kUnit;
      if constexpr (VEC) *reinterpret_cast<u32x4*>(bad) = u32x4{0u, 0u, 0u, 0u};
      else *reinterpret_cast<uint16_t*>(bad) = 0;
      continue;
    }
    const char* src = reinterpret_cast<const char*>(a.in.p[g]) + (int64_t)b * a.isb.b + (int64_t)h * a.isb.h +
                      t * a.isb.t + (int64_t)v * kUnit;
    char* dst = a.out + (int64_t)g * a.osb.g + (int64_t)b * a.osb.b + (int64_t)h * a.osb.h + (int64_t)j * a.osb.t +
                (int64_t)v * kUnit;
    if constexpr (VEC)
      __builtin_nontemporal_store(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src)), reinterpret_cast<u32x4*>(dst));
    else
      *reinterpret_cast<uint16_t*>(dst) = *reinterpret_cast<const uint16_t*>(src);
  }
}

// The same gather as 4 KiB work items (round 4): one 16-byte piece per thread, NO loop — blockIdx.x walks the output row of
// one (batch row, head) (blockIdx.z) in 256-piece steps, so a workgroup writes 4 KiB of contiguous output (256 / vecs token
// rows) and reads that many source rows: the launch shape of copy_rows_k, the fastest copy recipe measured on this chip
// (6.58 TB/s against 4.6-5.4 for grid-stride loops, profiles/r01e_microbench_calibration.txt). No division by n_idx per piece
// (the (b, h) row is grid dimension y, the tensor z); vecs is a power of two for every head_dim the library's other fast paths take.
__global__ __launch_bounds__(kBlock) void gather_rows_k(const GatherArgs a, const uint32_t vshift) {
  const uint32_t g = blockIdx.z, bh = blockIdx.y;  // dispatch order x, y, z: one tensor's rows are walked together before the next tensor's
  const uint32_t b = bh / a.H, h = bh - b * a.H;
  const uint32_t piece = blockIdx.x * kBlock + threadIdx.x;  // of this (b, h) row's n_idx * vecs pieces
  const uint32_t j = piece >> vshift, v = piece & ((1u << vshift) - 1u);
  if (j >= a.n_idx) return;
  const int64_t t = a.idx[j];
  char* dst = a.out + (int64_t)g * a.osb.g + (int64_t)b * a.osb.b + (int64_t)h * a.osb.h + (int64_t)j * a.osb.t + (int64_t)v * 16;
  u32x4 x = {0u, 0u, 0u, 0u};  // an index outside [0, T): a row of zeros, never an address
  if ((uint64_t)t < (uint64_t)a.T)
    x = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(a.in.p[g]) + (int64_t)b * a.isb.b +
                                                                  (int64_t)h * a.isb.h + t * a.isb.t + (int64_t)v * 16));
  __builtin_nontemporal_store(x, reinterpret_cast<u32x4*>(dst));
}

// ---------------------------------------------------------------------------- chunk mean-pool

struct PoolArgs {
  PtrTable in;
  Strides is;  // elements
  void* out;   // base of this launch's first group
  Strides os;  // elements
  uint32_t B, H, D;
  uint32_t T, Tout;
  uint32_t old_len, n_chunks, chunk;
  float chunk_f;  // (float)chunk_size: the divisor, also for the ragged last chunk
  int32_t nt_loads;
};

// independent 16-byte loads in flight per lane (raw packed registers: 4 VGPRs each for fp16/bf16)
template <int DT>
struct PoolBatch {
  static constexpr int n = DT == KVQ_F32 ? 8 : 16;
};

// Fast path: D % 8 == 0, 16-byte aligned rows. One lane owns 8 consecutive d of one output
// token; the D/8 lanes of a token read one contiguous row per step. fp32 accumulation is
// sequential in t (bit-reproducible, mirrored by the oracle).
// NTL: non-temporal loads, a COMPILE-TIME choice (a run-time `if (flag) load_nt else load` is merged by the compiler into
// plain loads: until the end of round 2 this kernel never issued a non-temporal load, whatever the tunable said)
template <int DT, bool NTL = true>
__global__ __launch_bounds__(kBlock) void chunk_pool_vec_k(const PoolArgs a, uint32_t items_per_g) {
  constexpr int NB = PoolBatch<DT>::n;
  const uint32_t g = blockIdx.y;
  const uint32_t DV = a.D >> 3;
  const int64_t tstride = a.is.t * Elem<DT>::size;
  // a grid-stride loop, launched with one item per thread
  for (uint32_t item = blockIdx.x * blockDim.x + threadIdx.x; item < items_per_g; item += gridDim.x * blockDim.x) {
    const uint32_t dv = item % DV;
    uint32_t r = item / DV;
    const uint32_t j = r % a.Tout;
    r /= a.Tout;
    const uint32_t h = r % a.H, b = r / a.H;
    const char* in = reinterpret_cast<const char*>(a.in.p[g]) +
                     ((int64_t)b * a.is.b + (int64_t)h * a.is.h + (int64_t)dv * 8) * Elem<DT>::size;
    char* out = reinterpret_cast<char*>(a.out) +
                ((int64_t)g * a.os.g + (int64_t)b * a.os.b + (int64_t)h * a.os.h + (int64_t)j * a.os.t +
                 (int64_t)dv * 8) * Elem<DT>::size;
    float acc[8];
    if (j >= a.n_chunks) {  // recent tail: exact copy of the raw words (a trip through fp32 quiets bf16 signalling NaNs)
      const u32x4* s = reinterpret_cast<const u32x4*>(in + (int64_t)(a.old_len + (j - a.n_chunks)) * tstride);
      u32x4* o = reinterpret_cast<u32x4*>(out);
#pragma unroll
      for (int w = 0; w < Elem<DT>::size / 2; ++w) o[w] = s[w];
      continue;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.0f;
    const uint32_t t0 = j * a.chunk;
    uint32_t n = a.old_len - t0;
    if (n > a.chunk) n = a.chunk;
    const char* p = in + (int64_t)t0 * tstride;
    uint32_t i = 0;
    for (; i + NB <= n; i += NB) {
      Vec8<DT> x[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        if constexpr (NTL) x[u].load_nt(p + (int64_t)(i + u) * tstride);
        else x[u].load(p + (int64_t)(i + u) * tstride);
      }
#pragma unroll
      for (int u = 0; u < NB; ++u)
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += x[u].get(k);
    }
    for (; i < n; ++i) {
      Vec8<DT> x;
      x.load(p + (int64_t)i * tstride);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += x.get(k);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = acc[k] / a.chunk_f;
    store8<DT, false>(out, acc);
  }
}

// One-wave workgroup = ONE output row (b, h, j): a pooled chunk or a copied tail row. The 64 lanes are G groups of
// DV = D / 8 lanes; group g owns rows RPG g .. RPG g + RPG - 1 of the chunk (chunk = G RPG rows), so the wave's RPG
// load instructions, ALL in flight at once, cover the chunk's chunk * D * 2 contiguous bytes exactly once and the
// wave ends — the access shape this memory system reads fastest (kvq_microbench poolpat: 7.1 TB/s against 5.8 for
// chunk_pool_vec_k's four-chunks-per-wave walk). The fp32 sum stays SEQUENTIAL in t, bit for bit the order of
// chunk_pool_vec_k and the oracle: G phases; in phase p every group adds its RPG rows to the sum it receives from the
// group below it (ds_bpermute), so after phase p group p holds the exact chain over rows 0 .. RPG (p + 1) - 1 (the other
// groups' values of that phase are never used), and group G - 1 ends with the whole chunk. Rows past a ragged last
// chunk's end enter as +0.0, which leaves an fp32 sum that started at +0.0 unchanged (the reference zero-pads too).
// (A variant without the redundant phases — 64 v_permlane16/32_swap instructions transpose the chunk so that every
// lane sums ONE dword of all 64 rows — was bit-identical and no faster: 5.76-5.85 vs 5.63-5.69 ms on the same box.)
template <int DT, int G, int RPG>
__global__ __launch_bounds__(64) void chunk_pool_wave_k(const PoolArgs a) {
  static_assert(DT != KVQ_F32, "16-bit element types");
  constexpr uint32_t DV = 64 / G;
  const uint32_t g = blockIdx.y;
  uint32_t r = blockIdx.x;
  const uint32_t j = r % a.Tout;
  r /= a.Tout;
  const uint32_t h = r % a.H, b = r / a.H;
  const uint32_t lane = threadIdx.x, lg = lane / DV, dv = lane % DV;
  const int64_t tstride = a.is.t * 2;
  const char* in = reinterpret_cast<const char*>(a.in.p[g]) + ((int64_t)b * a.is.b + (int64_t)h * a.is.h + (int64_t)dv * 8) * 2;
  char* out = reinterpret_cast<char*>(a.out) +
              ((int64_t)g * a.os.g + (int64_t)b * a.os.b + (int64_t)h * a.os.h + (int64_t)j * a.os.t + (int64_t)dv * 8) * 2;
  if (j >= a.n_chunks) {  // recent tail: exact copy (wave-uniform branch)
    if (lg == 0u)
      *reinterpret_cast<u32x4*>(out) = *reinterpret_cast<const u32x4*>(in + (int64_t)(a.old_len + (j - a.n_chunks)) * tstride);
    return;
  }
  const uint32_t t0 = j * a.chunk;
  uint32_t n = a.old_len - t0;
  if (n > a.chunk) n = a.chunk;  // >= 1
  // the chunk's valid rows as a buffer: rows past a ragged chunk's end are out of range and load as zeros
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(a.in.p[g]) + ((int64_t)b * a.is.b + (int64_t)h * a.is.h) * 2 + (int64_t)t0 * tstride), 0,
      (int)(n * (uint32_t)tstride), 0x00020000);
  u32x4 raw[RPG];
#pragma unroll
  for (int i = 0; i < RPG; ++i)  // all in flight
    raw[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (lg * RPG + i) * (uint32_t)tstride + dv * 16u, 0, 2);
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  f32x2 acc2[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) acc2[k] = f32x2{0.0f, 0.0f};
  // widen once, then packed fp32 adds (IEEE per component: the same sums as scalar adds, half the instructions —
  // with scalar adds the kernel measured 5.58-5.74 ms at config 5, packed 5.21 ms; widening inside every phase
  // instead, to save registers: 5.45 ms)
  f32x2 xf[RPG][4];
#pragma unroll
  for (int i = 0; i < RPG; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k)
      xf[i][k] = f32x2{Elem<DT>::widen((uint16_t)(raw[i][k] & 0xFFFFu)), Elem<DT>::widen((uint16_t)(raw[i][k] >> 16))};
#pragma unroll
  for (int ph = 0; ph < G; ++ph) {
    if (ph) {
#pragma unroll
      for (int k = 0; k < 4; ++k) acc2[k] = f32x2{__shfl_up(acc2[k][0], DV), __shfl_up(acc2[k][1], DV)};
    }
#pragma unroll
    for (int i = 0; i < RPG; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc2[k] += xf[i][k];
  }
  float acc[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    acc[2 * k] = acc2[k][0];
    acc[2 * k + 1] = acc2[k][1];
  }
  if (lg == (uint32_t)(G - 1)) {
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = acc[k] / a.chunk_f;
    store8<DT, false>(out, acc);
  }
}

// Generic path: any D / strides / alignment; one thread per output element.
template <int DT>
__global__ __launch_bounds__(kBlock) void chunk_pool_generic_k(const PoolArgs a, int64_t items_per_g) {
  const uint32_t g = blockIdx.y;
  const void* in = a.in.p[g];
  for (int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x; item < items_per_g;
       item += (int64_t)gridDim.x * kBlock) {
    const int64_t d = item % a.D;
    int64_t r = item / a.D;
    const int64_t j = r % a.Tout;
    r /= a.Tout;
    const int64_t h = r % a.H, b = r / a.H;
    const int64_t ibase = b * a.is.b + h * a.is.h + d;
    const int64_t o = (int64_t)g * a.os.g + b * a.os.b + h * a.os.h + j * a.os.t + d;
    if (j >= a.n_chunks) {  // recent tail: the element's raw bits
      typedef typename std::conditional<DT == KVQ_F32, uint32_t, uint16_t>::type word_t;
      reinterpret_cast<word_t*>(a.out)[o] = reinterpret_cast<const word_t*>(in)[ibase + (int64_t)(a.old_len + (j - a.n_chunks)) * a.is.t];
      continue;
    }
    const int64_t t0 = j * (int64_t)a.chunk;
    int64_t n = (int64_t)a.old_len - t0;
    if (n > a.chunk) n = a.chunk;
    float acc = 0.0f;
    for (int64_t i = 0; i < n; ++i) acc += load1<DT>(in, ibase + (t0 + i) * a.is.t);
    store1<DT>(a.out, o, acc / a.chunk_f);
  }
}

// ---------------------------------------------------------------------------- chunk summary inside the quantised store

// kvq_store_chunk_pool: codes and scale tables of ONE store, G groups in one allocation each (byte strides for the codes).
struct StorePoolArgs {
  const uint8_t* qin;
  Strides isb;  // bytes
  const float* sin;
  int64_t sin_g;  // floats
  uint8_t* qout;
  Strides osb;  // bytes
  float* sout;
  int64_t sout_g;
  uint32_t BH, H, D, Dq;
  uint32_t old_len, n_chunks, chunk, keep;
  float chunk_f, eps;
};

constexpr uint32_t kStoreTailRows = 16;  // kept tail tokens one workgroup copies

// x[t] = RN_dtype(float(code) * scale) — the dequantise kernels' expression — added to the lane's running fp32 sums
template <int DT, int BITS, class RAW, int EPP>
__device__ inline void store_pool_add(const RAW raw, const float s, float (&acc)[EPP]) {
  if constexpr (BITS == 8) {
#pragma unroll
    for (int k = 0; k < EPP; ++k) {
      const int v = (int)(int8_t)((raw[k >> 2] >> (8 * (k & 3))) & 0xFFu);
      acc[k] += Elem<DT>::round_trip(mul_exact((float)v, s));
    }
  } else {
#pragma unroll
    for (int k = 0; k < EPP; ++k) {  // even element = HIGH nibble of its byte
      const uint32_t byte = (raw[k >> 3] >> (8 * ((k >> 1) & 3))) & 0xFFu;
      const int v = (int)((k & 1) ? (byte & 0xFu) : (byte >> 4)) - 8;
      acc[k] += Elem<DT>::round_trip(mul_exact((float)v, s));
    }
  }
}

// The tail of kvq_store_chunk_pool: raw code bytes and raw scale words of kept tokens [r0, r0 + rows) — never requantised.
// UNIT 16: rows, strides and bases 16-byte aligned; UNIT 1: anything.
template <int UNIT, int NT>
__device__ inline void store_pool_tail(const StorePoolArgs& a, const uint8_t* qin, uint8_t* qout, const float* sin, float* sout,
                                       const uint32_t run) {
  const uint32_t r0 = run * kStoreTailRows;
  const uint32_t rows = a.keep - r0 < kStoreTailRows ? a.keep - r0 : kStoreTailRows;
  const uint32_t V = a.Dq / UNIT;
  const uint32_t items = a.BH * rows * V;
  for (uint32_t p = threadIdx.x; p < items; p += NT) {
    const uint32_t v = p % V;
    uint32_t r = p / V;
    const uint32_t row = r % rows, bh = r / rows;
    const uint32_t b = bh / a.H, h = bh - b * a.H;
    const uint8_t* src = qin + (int64_t)b * a.isb.b + (int64_t)h * a.isb.h + (int64_t)(a.old_len + r0 + row) * a.isb.t + (int64_t)v * UNIT;
    uint8_t* dst = qout + (int64_t)b * a.osb.b + (int64_t)h * a.osb.h + (int64_t)(a.n_chunks + r0 + row) * a.osb.t + (int64_t)v * UNIT;
    if constexpr (UNIT == 16)
      __builtin_nontemporal_store(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src)), reinterpret_cast<u32x4*>(dst));
    else
      *dst = *src;
  }
  if (threadIdx.x < rows)  // the scale's raw fp32 word
    reinterpret_cast<uint32_t*>(sout)[a.n_chunks + r0 + threadIdx.x] = reinterpret_cast<const uint32_t*>(sin)[a.old_len + r0 + threadIdx.x];
}

// Fast path: D % 32 == 0, 16-byte aligned rows, B * H * D <= 8192. One workgroup = ONE pooled token of one group (or a run of
// kept tail rows), so the abs-max over the whole [B,H,D] slice never leaves the workgroup: no workspace, no second pass.
// One lane owns PPT 16-byte code pieces (16 INT8 / 32 INT4 elements each) of the slice and walks the chunk's tokens in
// order: the fp32 sums are sequential in t from +0.0, the divide is IEEE, bit for bit kvq_dequant_*_tokens ->
// kvq_chunk_meanpool -> kvq_quant_*_tokens. The 16-byte loads of NB consecutive token rows are all issued (non-temporal:
// read once) before the first is used; the Dq / 16 lanes of a (b, h) row read that row's bytes of one token contiguously,
// and a lane's NB requests run through the chunk's contiguous chunk * Dq bytes. The pooled values stay in registers
// between the abs-max and the quantisation; each lane writes its 16 output bytes with one store.
// PB: bytes per piece, 16, or 8 for an INT4 slice of at most 32 16-byte pieces (Llama-3-8B's batch-1 V slice): half a wave
// would idle, and the kernel is bound by its per-element arithmetic (measured: 0.40 ms with 16-byte pieces against 0.20 ms
// for the INT8 store of twice the bytes).
template <int DT, int BITS, int NT, int PPT, int PB = 16>
__global__ __launch_bounds__(NT) void store_pool_fast_k(const StorePoolArgs a) {
  typedef typename std::conditional<PB == 16, u32x4, u32x2>::type raw_t;
  constexpr int EPP = PB * 8 / BITS;
  constexpr int NB = PPT == 1 ? 16 : 8;
  __shared__ float s_red[kBlock / kWave];
  const uint32_t g = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
  const uint8_t* qin = a.qin + (int64_t)g * a.isb.g;
  uint8_t* qout = a.qout + (int64_t)g * a.osb.g;
  const float* sin = a.sin + (int64_t)g * a.sin_g;
  float* sout = a.sout + (int64_t)g * a.sout_g;
  if (j >= a.n_chunks) {  // workgroup-uniform
    store_pool_tail<16, NT>(a, qin, qout, sin, sout, j - a.n_chunks);
    return;
  }
  const uint32_t V = a.Dq / PB, pieces = a.BH * V;
  const uint32_t t0 = j * a.chunk;
  uint32_t n = a.old_len - t0;
  if (n > a.chunk) n = a.chunk;  // >= 1
  const uint8_t* src[PPT];
  uint8_t* dst[PPT];
  bool on[PPT];
  float acc[PPT][EPP];
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const uint32_t p = tid + (uint32_t)k * NT;
    on[k] = p < pieces;
    const uint32_t pp = on[k] ? p : 0u;  // an idle lane re-reads piece 0 (in bounds) and writes nothing
    const uint32_t v = pp % V, bh = pp / V;
    const uint32_t b = bh / a.H, h = bh - b * a.H;
    src[k] = qin + (int64_t)b * a.isb.b + (int64_t)h * a.isb.h + (int64_t)t0 * a.isb.t + (int64_t)v * PB;
    dst[k] = qout + (int64_t)b * a.osb.b + (int64_t)h * a.osb.h + (int64_t)j * a.osb.t + (int64_t)v * PB;
#pragma unroll
    for (int e = 0; e < EPP; ++e) acc[k][e] = 0.0f;
  }
  const float* sc = sin + t0;
  uint32_t i = 0;
  for (; i + NB <= n; i += NB) {
    raw_t raw[NB][PPT];
    float s[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {  // all in flight
      s[u] = sc[i + u];
#pragma unroll
      for (int k = 0; k < PPT; ++k)
        raw[u][k] = __builtin_nontemporal_load(reinterpret_cast<const raw_t*>(src[k] + (int64_t)(i + u) * a.isb.t));
    }
#pragma unroll
    for (int u = 0; u < NB; ++u)
#pragma unroll
      for (int k = 0; k < PPT; ++k) store_pool_add<DT, BITS, raw_t, EPP>(raw[u][k], s[u], acc[k]);
  }
  if (i < n) {  // the rest of the chunk (a ragged last chunk, or chunk_size % NB): the same, row by row guarded
    raw_t raw[NB][PPT];
    float s[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (i + u < n) {
        s[u] = sc[i + u];
#pragma unroll
        for (int k = 0; k < PPT; ++k)
          raw[u][k] = __builtin_nontemporal_load(reinterpret_cast<const raw_t*>(src[k] + (int64_t)(i + u) * a.isb.t));
      }
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (i + u < n) {
#pragma unroll
        for (int k = 0; k < PPT; ++k) store_pool_add<DT, BITS, raw_t, EPP>(raw[u][k], s[u], acc[k]);
      }
    }
  }
  float m = 0.0f;
#pragma unroll
  for (int k = 0; k < PPT; ++k)
#pragma unroll
    for (int e = 0; e < EPP; ++e) {
      acc[k][e] = Elem<DT>::round_trip(acc[k][e] / a.chunk_f);  // the divisor is chunk_size for a ragged chunk too
      if (on[k]) m = max_nonneg(m, fabsf(acc[k][e]));  // a NaN mean (a pooled token with a NaN or inf scale) is kept
    }
  if constexpr (NT == kWave) m = wave_max(m);
  else m = block_max_nonneg(m, s_red);
  const float s32 = scale_of<BITS>(m, a.eps);
  if (tid == 0) sout[j] = Elem<DT>::round_trip(s32);
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    raw_t o = {};
    if constexpr (BITS == 8) {
#pragma unroll
      for (int e = 0; e < EPP; ++e) o[e >> 2] |= ((uint32_t)quant1<8>(acc[k][e], s32) & 0xFFu) << (8 * (e & 3));
    } else {
#pragma unroll
      for (int e = 0; e < EPP; e += 2) {
        const uint32_t hi = (uint32_t)(quant1<4>(acc[k][e], s32) + 8) & 0xFu, lo = (uint32_t)(quant1<4>(acc[k][e + 1], s32) + 8) & 0xFu;
        o[e >> 3] |= ((hi << 4) | lo) << (8 * ((e >> 1) & 3));
      }
    }
    if (on[k]) __builtin_nontemporal_store(o, reinterpret_cast<raw_t*>(dst[k]));
  }
}

constexpr uint32_t kStoreSliceMax = 8192;  // B * H * D one workgroup pools (the decode step's one-round-trip new-token limit)

// Generic path: any D / strides / alignment with B * H * D <= 8192. One workgroup per pooled token; one thread per element
// walks the chunk in t, the pooled values wait in LDS for the slice's abs-max.
template <int DT, int BITS>
__global__ __launch_bounds__(kBlock) void store_pool_generic_k(const StorePoolArgs a) {
  __shared__ float s_m[kStoreSliceMax];
  __shared__ float s_red[kBlock / kWave];
  const uint32_t g = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
  const uint8_t* qin = a.qin + (int64_t)g * a.isb.g;
  uint8_t* qout = a.qout + (int64_t)g * a.osb.g;
  const float* sin = a.sin + (int64_t)g * a.sin_g;
  float* sout = a.sout + (int64_t)g * a.sout_g;
  if (j >= a.n_chunks) {
    store_pool_tail<1, kBlock>(a, qin, qout, sin, sout, j - a.n_chunks);
    return;
  }
  const uint32_t t0 = j * a.chunk;
  uint32_t n = a.old_len - t0;
  if (n > a.chunk) n = a.chunk;
  const uint32_t n_el = a.BH * a.D;
  float m = 0.0f;
  for (uint32_t e = tid; e < n_el; e += kBlock) {
    const uint32_t d = e % a.D, bh = e / a.D;
    const uint32_t b = bh / a.H, h = bh - b * a.H;
    const uint8_t* col = qin + (int64_t)b * a.isb.b + (int64_t)h * a.isb.h + (int64_t)t0 * a.isb.t + (BITS == 8 ? d : d >> 1);
    float acc = 0.0f;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t byte = col[(int64_t)i * a.isb.t];
      const int v = BITS == 8 ? (int)(int8_t)byte : (int)((d & 1) ? (byte & 0x0Fu) : (byte >> 4)) - 8;
      acc += Elem<DT>::round_trip(mul_exact((float)v, sin[t0 + i]));
    }
    const float mean = Elem<DT>::round_trip(acc / a.chunk_f);
    s_m[e] = mean;
    m = max_nonneg(m, fabsf(mean));
  }
  m = block_max_nonneg(m, s_red);  // its barriers also publish s_m
  const float s32 = scale_of<BITS>(m, a.eps);
  if (tid == 0) sout[j] = Elem<DT>::round_trip(s32);
  const uint32_t n_bytes = a.BH * a.Dq;
  for (uint32_t i = tid; i < n_bytes; i += kBlock) {
    const uint32_t c = i % a.Dq, bh = i / a.Dq;
    const uint32_t b = bh / a.H, h = bh - b * a.H;
    uint8_t byte;
    if constexpr (BITS == 8) {
      byte = (uint8_t)(int8_t)quant1<8>(s_m[bh * a.D + c], s32);
    } else {  // odd D: the pad nibble is 8, as kvq_quant_i4_tokens writes it
      const int hi = quant1<4>(s_m[bh * a.D + 2 * c], s32) + 8;
      const int lo = 2 * c + 1 < a.D ? quant1<4>(s_m[bh * a.D + 2 * c + 1], s32) + 8 : 8;
      byte = (uint8_t)(((hi & 0xF) << 4) | (lo & 0xF));
    }
    qout[(int64_t)b * a.osb.b + (int64_t)h * a.osb.h + (int64_t)j * a.osb.t + c] = byte;
  }
}

// ---------------------------------------------------------------------------- host side

static int common_checks(const void* in_base, const void* const* in_ptrs, const kvq_strides_t* in_st, void* out,
                         const kvq_strides_t* out_st, const kvq_dims_t* d, const char* name) {
  if (const int rc = check_group_call(in_st && out_st && out, in_base, in_ptrs, out, d, name)) return rc;
  if (d->B * d->H >= (int64_t(1) << 31) || d->T >= (int64_t(1) << 31) || d->D >= (int64_t(1) << 31)) {
    set_error("%s: dims too large", name);
    return KVQ_E_DIMS;
  }
  return 0;
}

// One validated, non-empty call of an eviction entry point: what the three share.
struct EvictCall {
  const void* in_base;
  const void* const* in_ptrs;
  char* out;
  Strides isb, osb;  // bytes
  bool vec_strides;  // input b, h, t and output g, b, h, t strides are multiples of 16 bytes
  int64_t esz, G, BH, H, T, D;
  hipStream_t st;
  const char* name;
};

static EvictCall evict_call(const char* name, const void* in_base, const void* const* in_ptrs, const kvq_strides_t* in_st,
                            void* out, const kvq_strides_t* out_st, int64_t esz, const kvq_dims_t* d, void* stream) {
  EvictCall c = {in_base, in_ptrs, static_cast<char*>(out), {in_st->g * esz, in_st->b * esz, in_st->h * esz, in_st->t * esz},
                 {out_st->g * esz, out_st->b * esz, out_st->h * esz, out_st->t * esz}, false, esz, d->G, d->B * d->H, d->H,
                 d->T, d->D, reinterpret_cast<hipStream_t>(stream), name};
  c.vec_strides = multiples_of(16, c.isb.b, c.isb.h, c.isb.t, c.osb.g, c.osb.b, c.osb.h, c.osb.t);
  return c;
}

// Launch chunk [g0, g0 + n) of a call: its pointer table, every entry advanced by extra_bytes, and its output base.
// aligned16: that base and every ADVANCED entry are 16-byte aligned (the caller's own pointers need not be).
static int chunk_ptrs(const EvictCall& c, int64_t g0, int64_t n, int64_t extra_bytes, PtrTable& in, char*& out, bool& aligned16) {
  if (const int rc = fill_ptrs(in, c.in_base, c.in_ptrs, g0, n, c.isb.g, extra_bytes, c.name)) return rc;
  out = c.out + g0 * c.osb.g;
  aligned16 = aligned(out, 16);
  for (int64_t i = 0; i < n && aligned16; ++i) aligned16 = aligned(in.p[i], 16);
  return 0;
}

// ---- routing of kvq_window_compact (copy_route, once per call; the family per launch chunk): first match wins ---------
//  refused  2^31 or more workgroups per group ("too many segments"), before any group pointer is looked at.
//  Vec      copy_rows_k<true>: segment bytes % 16 == 0, EvictCall::vec_strides (one_base: the input group stride too, which
//           the kernel then adds itself) and, per LAUNCH CHUNK, a 16-byte aligned output base and group pointers that are
//           16-byte aligned once ADVANCED to the first kept token (chunk_ptrs).
//  Scalar   copy_rows_k<false>: the rest, 2 bytes per thread and step.
// one_base: more groups than one pointer table holds, all in ONE allocation (a paged pool's blocks): the kernel adds
// g * stride itself, up to 65,535 groups per launch (PagedKVCache.get_kv at 32 K tokens: 1 launch per pool instead of 4).
enum class Copy { Vec, Scalar };

struct CopyRoute {
  Copy fam;  // of a launch chunk that chunk_ptrs finds aligned; any other chunk is Scalar
  uint32_t segs_per_bh, cps, one_base;  // CopyArgs' fields
  int64_t seg_bytes, blocks;            // blocks: workgroups per group
};

static int copy_route(const EvictCall& c, int64_t W, CopyRoute& r) {
  const bool tcontig = c.isb.t == c.D * c.esz && c.osb.t == c.D * c.esz;
  r.segs_per_bh = tcontig ? 1u : (uint32_t)W;
  r.seg_bytes = (tcontig ? W * c.D : c.D) * c.esz;
  r.cps = (uint32_t)((r.seg_bytes + kCopyChunk - 1) / kCopyChunk);
  r.blocks = c.BH * r.segs_per_bh * r.cps;
  if (r.blocks >= (int64_t(1) << 31)) {
    set_error("%s: too many segments", c.name);
    return KVQ_E_DIMS;
  }
  r.one_base = (c.in_base && c.G > kPtrsPerLaunch) ? 1u : 0u;
  r.fam = r.seg_bytes % 16 == 0 && c.vec_strides && (!r.one_base || c.isb.g % 16 == 0) ? Copy::Vec : Copy::Scalar;
  return 0;
}

static void launch_copy(const EvictCall& c, const CopyRoute& r, Copy fam, const CopyArgs& a, int64_t gn) {
  const dim3 grid((unsigned)r.blocks, (unsigned)gn);
  if (fam == Copy::Vec) KVQ_LAUNCH((copy_rows_k<true>), grid, dim3(kBlock), 0, c.st, a);
  else KVQ_LAUNCH((copy_rows_k<false>), grid, dim3(kBlock), 0, c.st, a);
}

// ---- routing of kvq_gather_tokens (gather_route, per launch chunk): first match wins -----------------------------------
//  A vector chunk (D * elem_size % 16 == 0, EvictCall::vec_strides, its output base and group pointers 16-byte aligned)
//  counts 16-byte pieces per token row (vecs), any other chunk 2-byte pieces.
//  refused  2^32 or more pieces per group ("too many elements per group"), in the chunk's own pieces.
//  Rows     gather_rows_k: a vector chunk, vecs a power of two, B * H < 65536 (a grid dimension), gather_rows on.
//  Vec      gather_tokens_k<true>: the other vector chunks.
//  Scalar   gather_tokens_k<false>: the rest.
enum class Gather { Rows, Vec, Scalar };

struct GatherRoute {
  Gather fam;
  uint32_t vecs;   // pieces per token row; Rows: vshift = log2(vecs)
  int32_t vshift;
  int64_t items;   // pieces per group
};

static int gather_route(const EvictCall& c, int64_t n_idx, bool chunk_aligned, GatherRoute& r) {
  const bool vec = c.D * c.esz % 16 == 0 && c.vec_strides && chunk_aligned;
  r.vecs = (uint32_t)(c.D * c.esz) / (vec ? 16u : 2u);
  r.items = c.BH * n_idx * (int64_t)r.vecs;
  if (r.items >= (int64_t(1) << 32)) {
    set_error("%s: too many elements per group", c.name);
    return KVQ_E_DIMS;
  }
  r.vshift = vec ? ilog2_exact((int64_t)r.vecs) : -1;  // -1: not a power of two
  r.fam = !vec ? Gather::Scalar : r.vshift >= 0 && c.BH < 65536 && tunables().gather_rows != 0 ? Gather::Rows : Gather::Vec;
  return 0;
}

static void launch_gather(const EvictCall& c, const GatherRoute& r, const GatherArgs& a, int64_t gn) {
  int64_t blocks = (r.items + kBlock - 1) / kBlock;
  if (blocks > 256 * 64) blocks = 256 * 64;
  const dim3 grid((unsigned)blocks, (unsigned)gn);
  if (r.fam == Gather::Rows)  // 4 KiB items, one piece per thread
    KVQ_LAUNCH(gather_rows_k, dim3((unsigned)(((int64_t)a.n_idx * r.vecs + kBlock - 1) / kBlock), (unsigned)c.BH, (unsigned)gn),
               dim3(kBlock), 0, c.st, a, (uint32_t)r.vshift);
  else if (r.fam == Gather::Vec) KVQ_LAUNCH((gather_tokens_k<true>), grid, dim3(kBlock), 0, c.st, a, (uint32_t)r.items);
  else KVQ_LAUNCH((gather_tokens_k<false>), grid, dim3(kBlock), 0, c.st, a, (uint32_t)r.items);
}

// ---- routing of kvq_chunk_meanpool (pool_route, once per call; the family per launch chunk): first match wins ----------
//  Generic  chunk_pool_generic_k<DT>: D % 8 != 0, EvictCall::vec_strides fails, 2^31 or more 8-element items per group —
//           and every LAUNCH CHUNK whose output base or group pointers are not 16-byte aligned, whatever the call's route.
//  Wave     chunk_pool_wave_k<DT, G, RPG>: pool_wave on, fp16 / bf16, D = 256 / 128 / 64 (G = 2 / 4 / 8 lane groups),
//           chunk_size = G * RPG with RPG = 8 or 16 rows per lane group, B * H * Tout < 2^31 (one wave per output row),
//           a chunk's bytes < 2^31 (32-bit offsets inside it).
//  Vec      chunk_pool_vec_k<DT, true>: the rest, one item per thread of 64-thread workgroups (measured on a config-5-shaped
//           launch: 6.04 TB/s; persistent grids of 2048 / 4096 / 16384 workgroups 5.85 / 5.94 / 6.00).
enum class Pool { Wave, Vec, Generic };

struct PoolRoute {
  Pool fam;              // of a launch chunk that chunk_ptrs finds aligned; any other chunk is Generic
  int lane_groups, rpg;  // Wave: G, RPG
  int64_t rows, items_vec, items_gen;  // per group: output rows B * H * Tout (Wave), times D/8 (Vec), times D (Generic)
};

static PoolRoute pool_route(const EvictCall& c, int dtype, int64_t chunk_size, int64_t Tout) {
  PoolRoute r = {Pool::Generic, 0, 0, c.BH * Tout, c.BH * Tout * (c.D / 8), c.BH * Tout * c.D};
  if (c.D % 8 != 0 || r.items_vec >= (int64_t(1) << 31) || !c.vec_strides) return r;
  r.lane_groups = c.D == 256 ? 2 : c.D == 128 ? 4 : c.D == 64 ? 8 : 0;
  r.rpg = r.lane_groups ? (int)(chunk_size / r.lane_groups) : 0;
  const bool wave = dtype != KVQ_F32 && tunables().pool_wave && r.lane_groups && chunk_size % r.lane_groups == 0 &&
                    (r.rpg == 8 || r.rpg == 16) && r.rows < (int64_t(1) << 31) && chunk_size * c.isb.t < (int64_t(1) << 31);
  r.fam = wave ? Pool::Wave : Pool::Vec;
  return r;
}

// chunk_pool_wave_k<DT, G, RPG> by [log2(G) - 1][RPG == 16]
template <int DT>
constexpr void (*kPoolWave[3][2])(PoolArgs) = {{chunk_pool_wave_k<DT, 2, 8>, chunk_pool_wave_k<DT, 2, 16>},
                                               {chunk_pool_wave_k<DT, 4, 8>, chunk_pool_wave_k<DT, 4, 16>},
                                               {chunk_pool_wave_k<DT, 8, 8>, chunk_pool_wave_k<DT, 8, 16>}};

static void launch_pool(const EvictCall& c, const PoolRoute& r, Pool fam, int dtype, const PoolArgs& a, int64_t gn) {
  by_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if (fam == Pool::Wave) {
      if constexpr (DT != KVQ_F32)
        KVQ_LAUNCH(kPoolWave<DT>[ilog2_exact(r.lane_groups) - 1][r.rpg == 16], dim3((unsigned)r.rows, (unsigned)gn), dim3(64), 0, c.st, a);
    } else if (fam == Pool::Vec) {
      KVQ_LAUNCH((chunk_pool_vec_k<DT, true>), dim3((unsigned)((r.items_vec + 63) / 64), (unsigned)gn), dim3(64), 0, c.st, a,
                 (uint32_t)r.items_vec);
    } else {
      int64_t blocks = (r.items_gen + kBlock - 1) / kBlock;
      if (blocks > 256 * 32) blocks = 256 * 32;
      KVQ_LAUNCH((chunk_pool_generic_k<DT>), dim3((unsigned)blocks, (unsigned)gn), dim3(kBlock), 0, c.st, a, r.items_gen);
    }
  });
}

// ---- routing of kvq_store_chunk_pool (store_pool_route, once per call): first match wins ----------------------------------
//  refused  B * H * D > 8192 ("slice of ... elements": the caller composes dequantise -> kvq_chunk_meanpool -> quantise).
//  Fast     store_pool_fast_k<DT, BITS, NT, PPT>: store_pool_fast on, D % 32 == 0, every byte stride of both code tensors a
//           multiple of 16, both bases 16-byte aligned. pieces = B * H * Dq / 16: NT = 64 up to 64 pieces, else 256 threads;
//           PPT = 2 pieces per thread past 256 pieces (INT8 only: INT4 has at most 256). An INT4 slice of at most 32 pieces
//           takes 8-byte pieces (PB = 8) so that a whole wave works.
//  Generic  store_pool_generic_k<DT, BITS>: the rest.
struct StorePoolRoute {
  bool fast;
  int nt, ppt, pb;
};

static StorePoolRoute store_pool_route(const StorePoolArgs& a, int bits) {
  StorePoolRoute r = {false, kBlock, 1, 16};
  r.fast = tunables().store_pool_fast != 0 && a.D % 32 == 0 && aligned(a.qin, 16) && aligned(a.qout, 16) &&
           multiples_of(16, a.isb.g, a.isb.b, a.isb.h, a.isb.t, a.osb.g, a.osb.b, a.osb.h, a.osb.t);
  if (!r.fast) return r;
  const int64_t pieces = (int64_t)a.BH * (a.Dq / 16);
  r.nt = pieces <= kWave ? kWave : kBlock;
  r.ppt = pieces > kBlock ? 2 : 1;
  r.pb = bits == 4 && pieces <= kWave / 2 ? 8 : 16;  // an INT4 slice that fills half a wave at most: 8-byte pieces
  return r;
}

template <int DT, int BITS>
static void launch_store_pool(const StorePoolRoute& r, const StorePoolArgs& a, const dim3 grid, hipStream_t st) {
  if (!r.fast) KVQ_LAUNCH((store_pool_generic_k<DT, BITS>), grid, dim3(kBlock), 0, st, a);
  else if (r.pb == 8) {
    if constexpr (BITS == 4) KVQ_LAUNCH((store_pool_fast_k<DT, 4, kWave, 1, 8>), grid, dim3(kWave), 0, st, a);
  } else if (r.nt == kWave) KVQ_LAUNCH((store_pool_fast_k<DT, BITS, kWave, 1>), grid, dim3(kWave), 0, st, a);
  else if (r.ppt == 1) KVQ_LAUNCH((store_pool_fast_k<DT, BITS, kBlock, 1>), grid, dim3(kBlock), 0, st, a);
  else if constexpr (BITS == 8) KVQ_LAUNCH((store_pool_fast_k<DT, 8, kBlock, 2>), grid, dim3(kBlock), 0, st, a);
}

// bytes from the base to one past the last byte of a [G,B,H,T,row] tensor with these byte strides
static int64_t extent_bytes(const Strides& s, int64_t G, int64_t B, int64_t H, int64_t T, int64_t row) {
  return (G - 1) * s.g + (B - 1) * s.b + (H - 1) * s.h + (T - 1) * s.t + row;
}

static bool ranges_overlap(const void* p, int64_t np, const void* q, int64_t nq) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + (uintptr_t)nq && b < a + (uintptr_t)np;
}

}  // namespace kvq

using namespace kvq;

extern "C" {

int kvq_window_compact(const void* in_base, const void* const* in_ptrs, const kvq_strides_t* in_st, void* out,
                       const kvq_strides_t* out_st, int elem_size, int64_t window, const kvq_dims_t* d,
                       void* stream) {
  const char* name = "kvq_window_compact";
  if (const int rc = common_checks(in_base, in_ptrs, in_st, out, out_st, d, name)) return rc;
  if ((elem_size != 2 && elem_size != 4) || window < 0) {
    set_error("%s: elem_size must be 2 or 4 and window >= 0", name);
    return KVQ_E_DIMS;
  }
  const int64_t W = window < d->T ? window : d->T;
  if (d->G * d->B * d->H * W * d->D == 0) return 0;
  const EvictCall c = evict_call(name, in_base, in_ptrs, in_st, out, out_st, elem_size, d, stream);
  CopyRoute r;
  if (const int rc = copy_route(c, W, r)) return rc;
  CopyArgs a;
  a.isb = c.isb; a.osb = c.osb; a.BH = (uint32_t)c.BH; a.H = (uint32_t)c.H;
  a.segs_per_bh = r.segs_per_bh; a.seg_bytes = r.seg_bytes; a.cps = r.cps; a.one_base = r.one_base;
  return for_launch_chunks(c.G, r.one_base ? 65535 : kPtrsPerLaunch, [&](int64_t g0, int64_t gn) -> int {
    bool chunk_aligned;
    if (const int rc = chunk_ptrs(c, g0, r.one_base ? 1 : gn, (c.T - W) * c.isb.t, a.in, a.out, chunk_aligned)) return rc;
    launch_copy(c, r, chunk_aligned ? r.fam : Copy::Scalar, a, gn);
    return check_launch(name);
  });
}

int kvq_gather_tokens(const void* in_base, const void* const* in_ptrs, const kvq_strides_t* in_st, void* out,
                      const kvq_strides_t* out_st, int elem_size, const int32_t* idx, int64_t n_idx,
                      const kvq_dims_t* d, void* stream) {
  const char* name = "kvq_gather_tokens";
  if (const int rc = common_checks(in_base, in_ptrs, in_st, out, out_st, d, name)) return rc;
  if ((elem_size != 2 && elem_size != 4) || n_idx < 0 || n_idx >= (int64_t(1) << 31)) {
    set_error("%s: elem_size must be 2 or 4 and 0 <= n_idx < 2^31", name);
    return KVQ_E_DIMS;
  }
  if (d->G * d->B * d->H * n_idx * d->D == 0) return 0;
  if (!idx) {
    set_error("%s: idx is NULL", name);
    return KVQ_E_NULL;
  }
  const EvictCall c = evict_call(name, in_base, in_ptrs, in_st, out, out_st, elem_size, d, stream);
  GatherArgs a;
  a.isb = c.isb; a.osb = c.osb; a.idx = idx;
  a.H = (uint32_t)c.H; a.n_idx = (uint32_t)n_idx; a.T = (uint32_t)c.T; a.row_bytes = (uint32_t)(c.D * c.esz);
  return for_launch_chunks(c.G, kPtrsPerLaunch, [&](int64_t g0, int64_t gn) -> int {
    bool chunk_aligned;
    if (const int rc = chunk_ptrs(c, g0, gn, 0, a.in, a.out, chunk_aligned)) return rc;
    GatherRoute r;
    if (const int rc = gather_route(c, n_idx, chunk_aligned, r)) return rc;
    a.vecs = r.vecs;
    launch_gather(c, r, a, gn);
    return check_launch(name);
  });
}

int kvq_chunk_meanpool(const void* in_base, const void* const* in_ptrs, const kvq_strides_t* in_st, void* out,
                       const kvq_strides_t* out_st, int dtype, int64_t chunk_size, int64_t keep_last,
                       const kvq_dims_t* d, void* stream) {
  const char* name = "kvq_chunk_meanpool";
  if (const int rc = common_checks(in_base, in_ptrs, in_st, out, out_st, d, name)) return rc;
  if (dtype != KVQ_F16 && dtype != KVQ_BF16 && dtype != KVQ_F32) {
    set_error("%s: unknown dtype %d", name, dtype);
    return KVQ_E_DTYPE;
  }
  if (chunk_size <= 0 || keep_last < 0 || chunk_size >= (int64_t(1) << 31)) {
    set_error("%s: chunk_size must be > 0 and keep_last >= 0", name);
    return KVQ_E_DIMS;
  }
  if (d->G * d->B * d->H * d->T * d->D == 0) return 0;
  const EvictCall c = evict_call(name, in_base, in_ptrs, in_st, out, out_st, dtype == KVQ_F32 ? 4 : 2, d, stream);
  const int64_t keep = keep_last < c.T ? keep_last : c.T;
  const int64_t old = c.T - keep;
  const int64_t n_chunks = old > 0 ? (old + chunk_size - 1) / chunk_size : 0;
  const int64_t Tout = n_chunks + keep;  // == T when old <= 0 (pure copy)
  const PoolRoute r = pool_route(c, dtype, chunk_size, Tout);
  PoolArgs a;
  a.is = to_strides(in_st); a.os = to_strides(out_st);
  a.B = (uint32_t)d->B; a.H = (uint32_t)c.H; a.D = (uint32_t)c.D; a.T = (uint32_t)c.T; a.Tout = (uint32_t)Tout;
  a.old_len = (uint32_t)(old > 0 ? old : 0); a.n_chunks = (uint32_t)n_chunks;
  a.chunk = (uint32_t)chunk_size; a.chunk_f = (float)chunk_size;  // the divisor, also for the ragged last chunk
  a.nt_loads = 1;  // non-temporal input loads ship
  return for_launch_chunks(c.G, kPtrsPerLaunch, [&](int64_t g0, int64_t gn) -> int {
    char* chunk_out;
    bool chunk_aligned;
    if (const int rc = chunk_ptrs(c, g0, gn, 0, a.in, chunk_out, chunk_aligned)) return rc;
    a.out = chunk_out;
    launch_pool(c, r, chunk_aligned ? r.fam : Pool::Generic, dtype, a, gn);
    return check_launch(name);
  });
}

int kvq_store_chunk_pool(int bits, const uint8_t* q_in, const kvq_strides_t* q_in_st, const float* scales_in,
                         int64_t scale_in_stride_g, uint8_t* q_out, const kvq_strides_t* q_out_st, float* scales_out,
                         int64_t scale_out_stride_g, int dtype, int64_t chunk_size, int64_t keep_last, float eps,
                         const kvq_dims_t* d, void* stream) {
  const char* name = "kvq_store_chunk_pool";
  if (!q_in || !q_in_st || !scales_in || !q_out || !q_out_st || !scales_out || !d) {
    set_error("%s: NULL argument", name);
    return KVQ_E_NULL;
  }
  if (const int rc = check_device(q_out, name)) return rc;
  if (const int rc = check_device(scales_out, name)) return rc;
  if (d->G < 0 || d->B < 0 || d->H < 0 || d->T < 0 || d->D < 0) {
    set_error("%s: bad dims: negative dim", name);
    return KVQ_E_DIMS;
  }
  if (d->B * d->H >= (int64_t(1) << 31) || d->T >= (int64_t(1) << 31) || d->D >= (int64_t(1) << 31)) {
    set_error("%s: dims too large", name);
    return KVQ_E_DIMS;
  }
  if (bits != 8 && bits != 4) {
    set_error("%s: bits must be 8 or 4, got %d", name, bits);
    return KVQ_E_DIMS;
  }
  if (dtype != KVQ_F16 && dtype != KVQ_BF16) {
    set_error("%s: dtype must be KVQ_F16 or KVQ_BF16, got %d", name, dtype);
    return KVQ_E_DTYPE;
  }
  if (chunk_size <= 0 || keep_last < 0 || chunk_size >= (int64_t(1) << 31)) {
    set_error("%s: chunk_size must be > 0 and keep_last >= 0", name);
    return KVQ_E_DIMS;
  }
  if (d->B * d->H * d->D > (int64_t)kStoreSliceMax) {
    set_error("%s: slice of %lld elements (B * H * D) exceeds the %u one workgroup pools; compose kvq_dequant_*_tokens, "
              "kvq_chunk_meanpool and kvq_quant_*_tokens instead", name, (long long)(d->B * d->H * d->D), kStoreSliceMax);
    return KVQ_E_DIMS;
  }
  if (d->G * d->B * d->H * d->T * d->D == 0) return 0;
  const int64_t keep = keep_last < d->T ? keep_last : d->T;
  const int64_t old = d->T - keep;
  const int64_t n_chunks = old > 0 ? (old + chunk_size - 1) / chunk_size : 0;
  const int64_t Tout = n_chunks + keep;
  const int64_t Dq = bits == 8 ? d->D : (d->D + 1) / 2;
  StorePoolArgs a;
  a.qin = q_in; a.isb = to_strides(q_in_st); a.sin = scales_in; a.sin_g = scale_in_stride_g;
  a.qout = q_out; a.osb = to_strides(q_out_st); a.sout = scales_out; a.sout_g = scale_out_stride_g;
  if (ranges_overlap(q_in, extent_bytes(a.isb, d->G, d->B, d->H, d->T, Dq), q_out, extent_bytes(a.osb, d->G, d->B, d->H, Tout, Dq)) ||
      ranges_overlap(scales_in, ((d->G - 1) * scale_in_stride_g + d->T) * 4, scales_out, ((d->G - 1) * scale_out_stride_g + Tout) * 4)) {
    set_error("%s: input and output overlap (the call is out of place)", name);
    return KVQ_E_DIMS;
  }
  a.BH = (uint32_t)(d->B * d->H); a.H = (uint32_t)d->H; a.D = (uint32_t)d->D; a.Dq = (uint32_t)Dq;
  a.old_len = (uint32_t)(old > 0 ? old : 0); a.n_chunks = (uint32_t)n_chunks; a.chunk = (uint32_t)chunk_size; a.keep = (uint32_t)keep;
  a.chunk_f = (float)chunk_size; a.eps = eps;
  const int64_t blocks = n_chunks + (keep + kStoreTailRows - 1) / kStoreTailRows;  // < 2^31 + 2^27
  const StorePoolRoute r = store_pool_route(a, bits);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return for_launch_chunks(d->G, 65535, [&](int64_t g0, int64_t gn) -> int {
    StorePoolArgs c = a;
    c.qin += g0 * a.isb.g; c.qout += g0 * a.osb.g; c.sin += g0 * a.sin_g; c.sout += g0 * a.sout_g;
    const dim3 grid((unsigned)blocks, (unsigned)gn);
    if (dtype == KVQ_F16) {
      if (bits == 8) launch_store_pool<KVQ_F16, 8>(r, c, grid, st);
      else launch_store_pool<KVQ_F16, 4>(r, c, grid, st);
    } else {
      if (bits == 8) launch_store_pool<KVQ_BF16, 8>(r, c, grid, st);
      else launch_store_pool<KVQ_BF16, 4>(r, c, grid, st);
    }
    return check_launch(name);
  });
}

}  // extern "C"

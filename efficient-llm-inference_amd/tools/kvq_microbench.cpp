// kvq_microbench — standalone HIP-event micro-benchmark of libkvq_hip.so on the GPU box.
//
//   kvq_microbench [dequant4|dequant8|quant4|quant8|qblock|pool|window|copy|mixed|flat|bufcheck|...|all] [iters]
//
// Times the shipped entry points at the Llama-3-8B seq-16K KV shape (BASELINE config 4: G=32, B=1, H=8, T=16384,
// D=128) and prints algorithmic GB/s (SURVEY §8d bytes), next to calibration kernels measured in the same process
// (a 16 B/lane copy, a 16 B/lane fill and the access patterns of the kernels without their arithmetic: the box's
// achievable stream rates).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "kvq_hip.h"

#define HIP_OK(x)                                                                      \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) {                                                            \
      fprintf(stderr, "%s:%d %s -> %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
      exit(2);                                                                         \
    }                                                                                  \
  } while (0)
#define KVQ_OK(x)                                                              \
  do {                                                                         \
    int rc_ = (x);                                                             \
    if (rc_ != 0) {                                                            \
      fprintf(stderr, "%s:%d %s -> %d %s\n", __FILE__, __LINE__, #x, rc_, kvq_last_error_string()); \
      exit(3);                                                                 \
    }                                                                          \
  } while (0)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void copy16_k(const u32x4* __restrict__ in, u32x4* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = in[i];
}
__global__ __launch_bounds__(256) void fill16_k(u32x4* __restrict__ out, int64_t n, uint32_t v) {
  u32x4 x = {v, v + 1, v + 2, v + 3};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = x;
}
__global__ __launch_bounds__(256) void fill16_nt_k(u32x4* __restrict__ out, int64_t n, uint32_t v) {
  u32x4 x = {v, v + 1, v + 2, v + 3};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    __builtin_nontemporal_store(x, &out[i]);
}
__global__ __launch_bounds__(256) void copy16_nt_k(const u32x4* __restrict__ in, u32x4* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    __builtin_nontemporal_store(__builtin_nontemporal_load(&in[i]), &out[i]);
}
// 1 byte read per 4 bytes written: the INT4 dequantise traffic mix with no arithmetic
__global__ __launch_bounds__(256) void expand4_k(const uint32_t* __restrict__ in, u32x4* __restrict__ out, int64_t n, int nt) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint32_t w = in[i];
    u32x4 x = {w, w ^ 1u, w ^ 2u, w ^ 3u};
    if (nt) __builtin_nontemporal_store(x, &out[i]);
    else out[i] = x;
  }
}
__global__ __launch_bounds__(256) void read16_k(const u32x4* __restrict__ in, uint32_t* sink, int64_t n) {
  u32x4 acc = {0, 0, 0, 0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) acc ^= in[i];
  if ((acc[0] ^ acc[1] ^ acc[2] ^ acc[3]) == 0x12345678u) sink[0] = 1;
}
// Does a workgroup read faster from SOME addresses than from others? One-wave workgroups, workgroup w reads the
// contiguous chunk (w + shift) mod n of VEC 16-byte vectors: the dispatcher deals workgroups round robin over the 8
// XCDs, so `shift` moves every XCD's chunks by shift * chunk bytes relative to the identity map.
template <int VEC>
__global__ __launch_bounds__(64) void read_chunk_shift_k(const u32x4* __restrict__ in, uint32_t* sink, uint32_t n_chunks, uint32_t shift) {
  uint32_t c = blockIdx.x + shift;
  if (c >= n_chunks) c -= n_chunks;
  const u32x4* p = in + (int64_t)c * VEC + threadIdx.x;
  u32x4 acc = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < VEC / 64; ++i) acc ^= __builtin_nontemporal_load(p + i * 64);
  if ((acc[0] ^ acc[1] ^ acc[2] ^ acc[3]) == 0x12345678u) sink[0] = 1;
}
// what v_permlane16_swap / v_permlane32_swap do to (a = lane, b = 100 + lane): printed by `permprobe`
__global__ void perm_probe_k(uint32_t* out) {
  typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
  const uint32_t l = threadIdx.x;
  const u32x2_t r16 = __builtin_amdgcn_permlane16_swap(l, 100u + l, false, false);
  const u32x2_t r32 = __builtin_amdgcn_permlane32_swap(l, 100u + l, false, false);
  out[l] = r16[0];
  out[64 + l] = r16[1];
  out[128 + l] = r32[0];
  out[192 + l] = r32[1];
}
// candidate read pattern for the chunk mean-pool: one-wave workgroup = ONE 16 KiB chunk (64 rows of 256 B); lane
// group g = lane / 16 owns rows 16 g .. 16 g + 15, so load instruction i fetches rows {i, 16 + i, 32 + i, 48 + i}
// (four 256-byte segments 4 KiB apart) and the wave's 16 instructions, all in flight, cover the chunk exactly once.
// ROWQ: instruction i fetches rows 4 i .. 4 i + 3 instead (1 KiB contiguous).
template <bool ROWQ>
__global__ __launch_bounds__(64) void read_chunk_rows_k(const u32x4* __restrict__ in, uint32_t* sink) {
  const uint32_t lane = threadIdx.x, g = lane >> 4, dv = lane & 15u;
  const u32x4* p = in + (int64_t)blockIdx.x * 1024 + dv;
  u32x4 x[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = __builtin_nontemporal_load(p + (ROWQ ? (4 * i + g) : (16 * g + i)) * 16);
  u32x4 acc = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 16; ++i) acc ^= x[i];
  if ((acc[0] ^ acc[1] ^ acc[2] ^ acc[3]) == 0x12345678u) sink[0] = 1;
}
// The quantise kernels' memory traffic without their arithmetic, two tile shapes (input [8 heads][T][128] fp16, 4 MiB
// per head; INT4 output [8][T][64] bytes):
//   COOP = false: one-wave workgroup = 4 tokens x 8 heads: 8 loads of 1 KiB (one per head), 2 stores covering 8
//                 pieces of 256 B (what quant_tokens_fused_k does)
//   COOP = true:  8-wave workgroup = 32 tokens x 8 heads, wave w = head w: 8 loads covering 8 KiB contiguous, one
//                 barrier (the abs-max exchange), 2 stores covering 2 KiB contiguous
// NVALU: dependent-free filler vector instructions between the loads' arrival and the stores (how much of the
// quantise kernel's ~500 vector instructions per wave the memory pipeline feels)
// one-wave tile + the real kernel's other habits: LDSOUT = the packed output goes through an LDS image (8 ds_write_b32,
// 2 ds_read_b128) before the two stores; CHAIN = that many dependent scalar loads (pointer chasing through a tiny
// device table) before the first data load, like the kernel's kernarg -> pointer table -> strides prologue
template <bool LDSOUT, int CHAIN>
__global__ __launch_bounds__(64) void rw_quant_tile2_k(const u32x4* const* __restrict__ table, u32x4* __restrict__ out, int64_t head_vec_in,
                                                       int64_t head_vec_out) {
  __shared__ __attribute__((aligned(16))) uint32_t s_o[512];
  const uint32_t lane = threadIdx.x;
  const u32x4* const* t = table;
#pragma unroll
  for (int c = 1; c < CHAIN; ++c) t = reinterpret_cast<const u32x4* const*>(__builtin_nontemporal_load(reinterpret_cast<const uintptr_t*>(t) + 1));
  const u32x4* in = t[0];
  const u32x4* p = in + (int64_t)blockIdx.x * 64 + lane;
  u32x4 x[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = __builtin_nontemporal_load(p + (int64_t)i * head_vec_in);
  u32x4 a0, a1;
  if (LDSOUT) {
#pragma unroll
    for (int i = 0; i < 8; ++i) s_o[i * 64 + lane] = x[i][0] ^ x[i][1] ^ x[i][2] ^ x[i][3];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    a0 = *reinterpret_cast<const u32x4*>(&s_o[lane * 4]);
    a1 = *reinterpret_cast<const u32x4*>(&s_o[256 + lane * 4]);
  } else {
    a0 = x[0] ^ x[1] ^ x[2] ^ x[3];
    a1 = x[4] ^ x[5] ^ x[6] ^ x[7];
  }
  u32x4* q = out + (int64_t)blockIdx.x * 16 + (lane & 15u);
  __builtin_nontemporal_store(a0, q + (int64_t)(lane >> 4) * head_vec_out);
  __builtin_nontemporal_store(a1, q + (int64_t)((lane >> 4) + 4) * head_vec_out);
}
// the one-wave tile with the REAL tensors' strides: input [G][8][T][128] fp16, output [G][8][T][64] bytes
// (blockIdx.x = tile of 4 tokens in the group, blockIdx.y = group): heads 4 MiB apart on the input side and 1 MiB
// apart on the output side instead of the flat microbench's 128 MiB / 32 MiB
__global__ __launch_bounds__(64) void rw_quant_tile_real_k(const u32x4* __restrict__ in, u32x4* __restrict__ out, uint32_t T) {
  const uint32_t lane = threadIdx.x;
  const int64_t hv_in = (int64_t)T * 16, hv_out = (int64_t)T * 4;
  const u32x4* p = in + (int64_t)blockIdx.y * 8 * hv_in + (int64_t)blockIdx.x * 64 + lane;
  u32x4 x[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = __builtin_nontemporal_load(p + (int64_t)i * hv_in);
  const u32x4 a0 = x[0] ^ x[1] ^ x[2] ^ x[3], a1 = x[4] ^ x[5] ^ x[6] ^ x[7];
  u32x4* q = out + (int64_t)blockIdx.y * 8 * hv_out + (int64_t)blockIdx.x * 16 + (lane & 15u);
  __builtin_nontemporal_store(a0, q + (int64_t)(lane >> 4) * hv_out);
  __builtin_nontemporal_store(a1, q + (int64_t)((lane >> 4) + 4) * hv_out);
}
// the dequantise kernels' memory traffic without their arithmetic: one-wave workgroup w reads QV 16-byte... no: reads
// IN_B bytes per lane (4 for the INT4 kernel: 4 x 4 B = 1 KiB per wave; 8 for INT8's 2 x 8 B) and writes OUTV 16-byte
// vectors per lane (4 KiB / 2 KiB per wave), all contiguous, non-temporal stores
template <int NLOAD, int LOADB, int NSTORE, bool NTL>
__global__ __launch_bounds__(64) void rw_dequant_chunk_k(const uint8_t* __restrict__ in, u32x4* __restrict__ out) {
  const uint32_t lane = threadIdx.x;
  const uint8_t* p = in + ((int64_t)blockIdx.x * NLOAD * 64 + lane) * LOADB;
  uint32_t w[NLOAD][2];
#pragma unroll
  for (int u = 0; u < NLOAD; ++u) {
    if (LOADB == 4) {
      w[u][0] = NTL ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p + (int64_t)u * 64 * LOADB)) : *reinterpret_cast<const uint32_t*>(p + (int64_t)u * 64 * LOADB);
      w[u][1] = 0;
    } else {
      const u32x2 v = NTL ? __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p + (int64_t)u * 64 * LOADB)) : *reinterpret_cast<const u32x2*>(p + (int64_t)u * 64 * LOADB);
      w[u][0] = v[0];
      w[u][1] = v[1];
    }
  }
  u32x4* q = out + (int64_t)blockIdx.x * NSTORE * 64 + lane;
#pragma unroll
  for (int s = 0; s < NSTORE; ++s) {
    const uint32_t a = w[s % NLOAD][0], b = w[s % NLOAD][1];
    __builtin_nontemporal_store(u32x4{a, a ^ b, a + s, b}, q + s * 64);
  }
}
// the INT8 tile: same 8 loads of 1 KiB, four stores covering 8 pieces of 512 B (NTS: non-temporal stores)
template <bool NTS>
__global__ __launch_bounds__(64) void rw_quant_tile_i8_k(const u32x4* __restrict__ in, u32x4* __restrict__ out, uint32_t T) {
  const uint32_t lane = threadIdx.x;
  const int64_t hv_in = (int64_t)T * 16, hv_out = (int64_t)T * 8;
  const u32x4* p = in + (int64_t)blockIdx.y * 8 * hv_in + (int64_t)blockIdx.x * 64 + lane;
  u32x4 x[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = __builtin_nontemporal_load(p + (int64_t)i * hv_in);
  u32x4* q = out + (int64_t)blockIdx.y * 8 * hv_out + (int64_t)blockIdx.x * 32 + (lane & 31u);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const u32x4 v = x[2 * j] ^ x[2 * j + 1];
    u32x4* dst = q + (int64_t)((lane >> 5) + 2 * j) * hv_out;
    if (NTS) __builtin_nontemporal_store(v, dst);
    else *dst = v;
  }
}
// Round 4: the one-wave tile's loads (8 x 1 KiB, one per head row, real strides) with the OUTPUT pieces of WAVES
// neighbouring tiles merged through LDS by a WAVES-wave workgroup: wave w still loads only its own 4-token tile, writes
// its 4 B (INT4) / 8 B (INT8) per lane and row into an LDS image [8 rows][WAVES x 4 tokens], ONE workgroup barrier, then
// every wave stores whole 1-KiB instructions of the image: a row's run is WAVES x 256 B (INT4) / WAVES x 512 B (INT8)
// contiguous instead of 256 / 512 B. pad_in / pad_out: extra tokens in the row strides (the stride experiment).
template <int WAVES, int BITS>
__global__ __launch_bounds__(WAVES * 64) void rw_quant_tile_wg_k(const u32x4* __restrict__ in, u32x4* __restrict__ out, uint32_t T,
                                                                 uint32_t pad_in, uint32_t pad_out) {
  constexpr int QW = BITS / 4;                   // dwords per lane and row (INT4 1, INT8 2)
  constexpr int ROWV = WAVES * 4 * BITS;         // 16-byte vectors of one row's merged run (INT4: WAVES x 16)
  constexpr int NI = BITS / 2;                   // store instructions per wave (INT4 2, INT8 4)
  __shared__ __attribute__((aligned(16))) uint32_t s_o[8 * WAVES * 64 * QW];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const int64_t hv_in = (int64_t)(T + pad_in) * 16, hv_out = (int64_t)(T + pad_out) * BITS;  // INT4: 4 vectors per token, INT8: 8
  const u32x4* p = in + (int64_t)blockIdx.y * 8 * hv_in + ((int64_t)blockIdx.x * WAVES + w) * 64 + lane;
  u32x4 x[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = __builtin_nontemporal_load(p + (int64_t)i * hv_in);
  u32x4 all = x[0];
#pragma unroll
  for (int i = 1; i < 8; ++i) all ^= x[i];     // like the abs-max: nothing leaves before every load is back
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint32_t* d = &s_o[((i * WAVES + w) * 64 + lane) * QW];
    d[0] = x[i][0] ^ all[1];
    if (QW == 2) d[1] = x[i][2] ^ all[3];
  }
  if (WAVES > 1) __syncthreads();
  else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  u32x4* q = out + (int64_t)blockIdx.y * 8 * hv_out + (int64_t)blockIdx.x * ROWV;
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const uint32_t f = (w * NI + j) * 64 + lane;  // vector of the image, row-major
    const u32x4 v = *reinterpret_cast<const u32x4*>(&s_o[f * 4]);
    __builtin_nontemporal_store(v, q + (int64_t)(f / ROWV) * hv_out + f % ROWV);
  }
}
template <bool COOP, int NVALU = 0>
__global__ __launch_bounds__(COOP ? 512 : 64) void rw_quant_tile_k(const u32x4* __restrict__ in, u32x4* __restrict__ out, int64_t head_vec_in,
                                                                   int64_t head_vec_out) {
  __shared__ uint32_t s_x[8];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  u32x4 x[8];
  if (COOP) {
    const u32x4* p = in + (int64_t)wave * head_vec_in + (int64_t)blockIdx.x * 512 + lane;  // 32 tokens x 16 vectors
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = __builtin_nontemporal_load(p + i * 64);
  } else {
    const u32x4* p = in + (int64_t)blockIdx.x * 64 + lane;  // 4 tokens x 16 vectors per head
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = __builtin_nontemporal_load(p + (int64_t)i * head_vec_in);
  }
  u32x4 acc = x[0];
#pragma unroll
  for (int i = 1; i < 8; ++i) acc ^= x[i];
  if constexpr (NVALU > 0) {
    float f[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = __uint_as_float(x[k][0] & 0x3FFFFFFFu);
#pragma unroll
    for (int it = 0; it < NVALU / 8; ++it)
#pragma unroll
      for (int k = 0; k < 8; ++k) f[k] = __builtin_fmaf(f[k], 1.0009765625f, 0.5f);  // 8 independent chains
    acc[2] ^= __float_as_uint(((f[0] + f[1]) + (f[2] + f[3])) + ((f[4] + f[5]) + (f[6] + f[7])));
  }
  if (COOP) {
    if (lane == 0) s_x[wave] = acc[0];
    __syncthreads();
    acc[1] ^= s_x[(wave + 1) & 7];
    u32x4* q = out + (int64_t)wave * head_vec_out + (int64_t)blockIdx.x * 128 + lane;  // 32 tokens x 4 vectors
    __builtin_nontemporal_store(acc, q);
    __builtin_nontemporal_store(acc ^ x[3], q + 64);
  } else {
    // 8 pieces of 256 B = 16 lanes each: lane -> (head = lane / 16 + 4 j, vector lane % 16)
    u32x4* q = out + (int64_t)blockIdx.x * 16 + (lane & 15u);
    __builtin_nontemporal_store(acc, q + (int64_t)(lane >> 4) * head_vec_out);
    __builtin_nontemporal_store(acc ^ x[3], q + (int64_t)((lane >> 4) + 4) * head_vec_out);
  }
}
// write ceiling with the launch shape of the dequantise kernel: one-wave workgroup w fills the contiguous chunk w of
// VEC 16-byte vectors (non-temporal or write-back stores)
template <int VEC, bool NT>
__global__ __launch_bounds__(64) void fill_chunk_k(u32x4* __restrict__ out, uint32_t v) {
  u32x4* p = out + (int64_t)blockIdx.x * VEC + threadIdx.x;
  const u32x4 x = {v, v + 1, v + 2, v + 3};
#pragma unroll
  for (int i = 0; i < VEC / 64; ++i) {
    if (NT) __builtin_nontemporal_store(x, p + i * 64);
    else p[i * 64] = x;
  }
}
// fill through a buffer descriptor with an explicit cache-policy immediate (aux: 1 = sc0, 2 = nt, 16 = sc1 and sums)
template <int AUX>
__global__ __launch_bounds__(64) void fill_chunk_aux_k(u32x4* __restrict__ out, uint32_t v) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(out + (int64_t)blockIdx.x * 256, 0, 4096, 0x00020000);
  const u32x4 x = {v, v + 1, v + 2, v + 3};
#pragma unroll
  for (int i = 0; i < 4; ++i) __builtin_amdgcn_raw_buffer_store_b128(x, rs, (i * 64 + threadIdx.x) * 16u, 0, AUX);
}
// The quantise tile's read pattern without anything else: one-wave workgroup w reads S segments of LVEC 16-byte
// vectors, segment s at s * seg_stride + w * LVEC (S = 8 heads 4 MiB apart, L = tokens per tile * 256 B). All loads
// of the workgroup are in flight together (non-temporal).
template <int S, int LVEC>
__global__ __launch_bounds__(64) void read_segments_k(const u32x4* __restrict__ in, uint32_t* sink, int64_t seg_stride_vec) {
  const u32x4* p = in + (int64_t)blockIdx.x * LVEC + threadIdx.x;
  u32x4 x[S * (LVEC / 64)];
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int i = 0; i < LVEC / 64; ++i) x[s * (LVEC / 64) + i] = __builtin_nontemporal_load(p + (int64_t)s * seg_stride_vec + i * 64);
  u32x4 acc = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < S * (LVEC / 64); ++k) acc ^= x[k];
  if ((acc[0] ^ acc[1] ^ acc[2] ^ acc[3]) == 0x12345678u) sink[0] = 1;
}
// copy recipes: U independent 16-byte loads per thread, then U stores (NT optional); one tile per block
template <int BLOCK, int U, bool NT>
__global__ __launch_bounds__(BLOCK) void copy16_tile_k(const u32x4* __restrict__ in, u32x4* __restrict__ out, int64_t n) {
  const int64_t base = (int64_t)blockIdx.x * BLOCK * U + threadIdx.x;
  u32x4 v[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t i = base + (int64_t)u * BLOCK;
    if (i < n) v[u] = NT ? __builtin_nontemporal_load(&in[i]) : in[i];
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t i = base + (int64_t)u * BLOCK;
    if (i < n) {
      if (NT) __builtin_nontemporal_store(v[u], &out[i]);
      else out[i] = v[u];
    }
  }
}
// read pattern of the chunk mean-pool kernel without its arithmetic: each 16-lane group streams
// 64 rows of 256 B (one chunk = 16 KiB), a wave covers 4 chunks -> every wave load touches four
// 256-byte segments 16 KiB apart. batch = loads in flight per lane.
template <int BATCH>
__global__ __launch_bounds__(256) void read_seg_k(const u32x4* __restrict__ in, uint32_t* sink, int64_t n_chunks) {
  const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t chunk = item >> 4;
  if (chunk >= n_chunks) return;
  const u32x4* p = in + chunk * 1024 + (item & 15);  // 16 KiB per chunk = 1024 vectors; row = 16 vectors
  u32x4 acc = {0, 0, 0, 0};
  for (int i = 0; i < 64; i += BATCH) {
    u32x4 x[BATCH];
#pragma unroll
    for (int u = 0; u < BATCH; ++u) x[u] = p[(i + u) * 16];
#pragma unroll
    for (int u = 0; u < BATCH; ++u) acc ^= x[u];
  }
  if ((acc[0] ^ acc[1] ^ acc[2] ^ acc[3]) == 0x12345678u) sink[0] = 1;
}
// the same bytes per wave (4 chunks of 16 KiB) with every wave-level load instruction ONE contiguous 1 KiB
// (4 consecutive rows of one chunk; the instruction stream cycles over the wave's 4 chunks)
template <int BATCH>
__global__ __launch_bounds__(64) void read_seg_rows_k(const u32x4* __restrict__ in, uint32_t* sink, int64_t n_chunks) {
  const int64_t wave = blockIdx.x;
  const int lane = threadIdx.x, g = lane >> 4, x = lane & 15;
  if (wave * 4 + 3 >= n_chunks) return;
  const u32x4* p = in + wave * 4 * 1024 + g * 16 + x;
  u32x4 acc = {0, 0, 0, 0};
  for (int b = 0; b < 64 / (BATCH / 4 * 4); ++b) {  // BATCH loads cover BATCH / 4 row quads of each of the 4 chunks
    u32x4 v[BATCH];
#pragma unroll
    for (int u = 0; u < BATCH; ++u) v[u] = p[(u & 3) * 1024 + (b * (BATCH / 4) + (u >> 2)) * 64];
#pragma unroll
    for (int u = 0; u < BATCH; ++u) acc ^= v[u];
  }
  if ((acc[0] ^ acc[1] ^ acc[2] ^ acc[3]) == 0x12345678u) sink[0] = 1;
}
__global__ void rand_fill_k(uint32_t* p, int64_t n_words, uint32_t seed) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * 256) {
    uint32_t x = (uint32_t)i * 2654435761u + seed;
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    p[i] = x;
  }
}
// fp16 N(0,1) values (Box-Muller on hashed bits). A coarse lattice (e.g. sums of a few bytes)
// makes x / scale hit exact half-integers constantly, which is not what KV tensors look like
// and sends the quantise kernel down its rare exact-division path.
__global__ void rand_f16_k(uint16_t* p, int64_t n, uint32_t seed) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    uint32_t x = (uint32_t)i * 2654435761u + seed;
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    uint32_t y = x * 747796405u + 2891336453u;
    y ^= y >> 15; y *= 0x2c1b3c6du; y ^= y >> 12;
    const float u1 = ((x >> 8) + 1) * (1.0f / 16777217.0f), u2 = (y >> 8) * (1.0f / 16777216.0f);
    const float g = sqrtf(-2.0f * __logf(u1)) * __cosf(6.2831853f * u2);
    _Float16 h = (_Float16)g;
    __builtin_memcpy(&p[i], &h, 2);
  }
}

struct Timer {
  hipEvent_t a, b;
  Timer() { HIP_OK(hipEventCreate(&a)); HIP_OK(hipEventCreate(&b)); }
  template <class F>
  double ms_per(F f, int iters, int warm = 3) {
    for (int i = 0; i < warm; ++i) f();
    HIP_OK(hipEventRecord(a, 0));
    for (int i = 0; i < iters; ++i) f();
    HIP_OK(hipEventRecord(b, 0));
    HIP_OK(hipEventSynchronize(b));
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, a, b));
    return ms / iters;
  }
};

// bufcheck: the range check the MFMA attention kernel relies on (kvq_attn.hip): a raw buffer load
// whose vector offset lies at or beyond num_records returns 0 and touches nothing.
__global__ void bufcheck_k(const uint8_t* base, uint32_t valid_bytes, uint32_t* out) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(base), 0, (int)valid_bytes, 0x00020000);
  const uint32_t off = threadIdx.x * 16u;  // 64 lanes x 16 B = 1 KiB; valid_bytes = 512: lanes 32.. are out of range
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 2);
  const uint32_t b = __builtin_amdgcn_raw_buffer_load_b32(r, off + 8u, 0, 2);
  const uint32_t c = (uint32_t)(uint16_t)__builtin_amdgcn_raw_buffer_load_b16(r, off + 2u, 0, 2);
  out[threadIdx.x * 3 + 0] = a[0] | a[1] | a[2] | a[3];
  out[threadIdx.x * 3 + 1] = b;
  out[threadIdx.x * 3 + 2] = c;
}

static int64_t G = 32, B = 1, H = 8, T = 16384, D = 128;  // override: KVQ_G / KVQ_T (G*T kept = 524288 by the caller)

int main(int argc, char** argv) {
  std::string what = argc > 1 ? argv[1] : "all";
  if (const char* tv = getenv("KVQ_TUNABLES")) {  // "key=value,key=value": kvq_set_tunable before anything runs
    std::string s = tv;
    size_t pos = 0;
    while (pos < s.size()) {
      size_t end = s.find(',', pos);
      if (end == std::string::npos) end = s.size();
      const std::string kv = s.substr(pos, end - pos);
      const size_t eq = kv.find('=');
      if (eq != std::string::npos) {
        if (kvq_set_tunable(kv.substr(0, eq).c_str(), atoll(kv.substr(eq + 1).c_str())) != 0) {
          fprintf(stderr, "unknown tunable %s\n", kv.c_str());
          return 2;
        }
        printf("# tunable %s\n", kv.c_str());
      }
      pos = end + 1;
    }
  }
  int iters = argc > 2 ? atoi(argv[2]) : 20;
  if (getenv("KVQ_G")) G = atoll(getenv("KVQ_G"));
  if (getenv("KVQ_T")) T = atoll(getenv("KVQ_T"));
  if (getenv("KVQ_B")) B = atoll(getenv("KVQ_B"));
  if (getenv("KVQ_H")) H = atoll(getenv("KVQ_H"));
  if (getenv("KVQ_D")) D = atoll(getenv("KVQ_D"));  // multiple of 8
  if (what == "bufcheck") {
    uint8_t* buf;
    uint32_t* out;
    HIP_OK(hipMalloc(&buf, 4096));
    HIP_OK(hipMalloc(&out, 64 * 3 * 4));
    HIP_OK(hipMemset(buf, 0xAB, 4096));
    bufcheck_k<<<1, 64>>>(buf, 512, out);
    uint32_t h[64 * 3];
    HIP_OK(hipMemcpy(h, out, sizeof(h), hipMemcpyDeviceToHost));
    int bad = 0;
    for (int l = 0; l < 64; ++l) {
      const bool in = l < 32;
      const uint32_t e128 = in ? 0xABABABABu : 0u, e32 = in ? 0xABABABABu : 0u, e16 = in ? 0xABABu : 0u;
      if (h[3 * l] != e128 || h[3 * l + 1] != e32 || h[3 * l + 2] != e16) {
        ++bad;
        printf("lane %d: got %08x %08x %04x expected %08x %08x %04x\n", l, h[3 * l], h[3 * l + 1], h[3 * l + 2], e128, e32, e16);
      }
    }
    printf("bufcheck: %s (lanes 0..31 in range read the fill pattern, lanes 32..63 out of range read 0)\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
  }
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, 0));
  printf("# device %s CUs=%d  shape G=%lld B=%lld H=%lld T=%lld D=%lld iters=%d\n", prop.gcnArchName,
         prop.multiProcessorCount, (long long)G, (long long)B, (long long)H, (long long)T, (long long)D, iters);
  const int64_t N = G * B * H * T * D;  // 536,870,912 elements
  Timer tm;

  // Rotating buffers: consecutive launches never touch the same lines, so the 256 MiB Infinity
  // Cache cannot serve re-reads (a single 256 MiB INT4 input re-read every iteration does stay
  // resident and inflates the rate: profiles/r01a_microbench_warm_cache.txt).
  constexpr int NBUF = 4;
  void *q8s[NBUF], *q4s[NBUF], *outs[2], *in16s[2];
  float *scales, *ws;
  for (int i = 0; i < NBUF; ++i) {
    HIP_OK(hipMalloc(&q8s[i], N));
    HIP_OK(hipMalloc(&q4s[i], N / 2));
    rand_fill_k<<<4096, 256>>>((uint32_t*)q8s[i], N / 4, 1u + i);
    rand_fill_k<<<4096, 256>>>((uint32_t*)q4s[i], N / 8, 20u + i);
  }
  for (int i = 0; i < 2; ++i) {
    HIP_OK(hipMalloc(&outs[i], N * 2));
    HIP_OK(hipMalloc(&in16s[i], N * 2));
    rand_f16_k<<<4096, 256>>>((uint16_t*)in16s[i], N, 3u + i);
  }
  HIP_OK(hipMalloc(&scales, G * T * 4));
  HIP_OK(hipMalloc(&ws, G * T * 4));
  int rot = 0;
  void *q8 = q8s[0], *q4 = q4s[0], *out = outs[0], *in16 = in16s[0];
  auto rotate = [&] {
    ++rot;
    q8 = q8s[rot % NBUF];
    q4 = q4s[rot % NBUF];
    out = outs[rot % 2];
    in16 = in16s[rot % 2];
  };
  {
    std::vector<float> s(G * T);
    for (size_t i = 0; i < s.size(); ++i) s[i] = 0.01f + 1e-6f * (float)(i % 977);
    HIP_OK(hipMemcpy(scales, s.data(), s.size() * 4, hipMemcpyHostToDevice));
  }
  HIP_OK(hipDeviceSynchronize());

  kvq_dims_t dims = {G, B, H, T, D};
  kvq_strides_t s_full = {B * H * T * D, H * T * D, T * D, D};
  kvq_strides_t s_half = {B * H * T * D / 2, H * T * D / 2, T * D / 2, D / 2};

  if (what == "affinity") {  // read bandwidth vs the offset between a workgroup's XCD and its chunk's address
    const int64_t bytes = N * 2;
#define RUN_AFF(VEC)                                                                                              \
  for (uint32_t shift : {0u, 1u, 2u, 3u, 4u, 5u, 6u, 7u, 8u, 64u}) {                                              \
    const uint32_t n_chunks = (uint32_t)(bytes / ((int64_t)VEC * 16));                                            \
    double best = 1e9;                                                                                            \
    for (int rep = 0; rep < 3; ++rep) {                                                                           \
      const double ms = tm.ms_per([&] { rotate(); read_chunk_shift_k<VEC><<<n_chunks, 64>>>((const u32x4*)in16, (uint32_t*)ws, n_chunks, shift); }, iters); \
      best = ms < best ? ms : best;                                                                               \
    }                                                                                                             \
    printf("calib affinity chunk=%6d B shift=%2u chunks  %8.3f ms  %8.1f GB/s (r)\n", VEC * 16, shift, best, 1.0 * bytes / best / 1e6); \
  }
    RUN_AFF(64) RUN_AFF(128) RUN_AFF(256) RUN_AFF(512) RUN_AFF(1024)
#undef RUN_AFF
  }
  if (what == "permprobe") {
    perm_probe_k<<<1, 64>>>((uint32_t*)ws);
    uint32_t h[256];
    HIP_OK(hipMemcpy(h, ws, sizeof(h), hipMemcpyDeviceToHost));
    const char* names[4] = {"permlane16_swap[0]", "permlane16_swap[1]", "permlane32_swap[0]", "permlane32_swap[1]"};
    for (int k = 0; k < 4; ++k) {
      printf("permprobe %s:", names[k]);
      for (int l = 0; l < 64; l += 8) printf(" l%d=%u", l, h[64 * k + l]);
      printf("\n");
    }
  }
  if (what == "flat") {  // the reference's two entry points on one large contiguous buffer (one scalar scale)
    for (int rep = 0; rep < 3; ++rep) {
      double ms = tm.ms_per([&] { rotate(); KVQ_OK(kvq_dequant_i4_f16_flat((const uint8_t*)q4, 0.0123f, out, N / 2, D / 2, D, 0)); }, iters);
      printf("flat dequant_i4_f16  %8.3f ms  %8.1f GB/s  frac8T=%.3f\n", ms, 2.5 * N / ms / 1e6, 2.5 * N / ms / 1e6 / 8000.0);
      ms = tm.ms_per([&] { rotate(); KVQ_OK(kvq_dequant_i8_f16_flat((const int8_t*)q8, 0.0123f, out, N, 0)); }, iters);
      printf("flat dequant_i8_f16  %8.3f ms  %8.1f GB/s  frac8T=%.3f\n", ms, 3.0 * N / ms / 1e6, 3.0 * N / ms / 1e6 / 8000.0);
    }
  }
  if (what == "dequantpat") {  // INT4: 1 KiB in / 4 KiB out per wave; INT8: 1 KiB in / 2 KiB out per wave
    for (int rep = 0; rep < 3; ++rep) {
      double ms = tm.ms_per([&] { rotate(); rw_dequant_chunk_k<4, 4, 4, false><<<(unsigned)(N / 2048), 64>>>((const uint8_t*)q4, (u32x4*)out); }, iters);
      printf("calib dequantpat INT4 traffic (1 KiB in, 4 KiB out per wave)            %8.3f ms  %8.1f GB/s\n", ms, 2.5 * N / ms / 1e6);
      ms = tm.ms_per([&] { rotate(); rw_dequant_chunk_k<4, 4, 4, true><<<(unsigned)(N / 2048), 64>>>((const uint8_t*)q4, (u32x4*)out); }, iters);
      printf("calib dequantpat INT4 traffic, non-temporal loads                        %8.3f ms  %8.1f GB/s\n", ms, 2.5 * N / ms / 1e6);
      ms = tm.ms_per([&] { rotate(); rw_dequant_chunk_k<2, 8, 2, true><<<(unsigned)(N / 1024), 64>>>((const uint8_t*)q8, (u32x4*)out); }, iters);
      printf("calib dequantpat INT8 traffic (1 KiB in, 2 KiB out per wave, nt loads)   %8.3f ms  %8.1f GB/s\n", ms, 3.0 * N / ms / 1e6);
      ms = tm.ms_per([&] { rotate(); rw_dequant_chunk_k<4, 8, 4, true><<<(unsigned)(N / 2048), 64>>>((const uint8_t*)q8, (u32x4*)out); }, iters);
      printf("calib dequantpat INT8 traffic (2 KiB in, 4 KiB out per wave, nt loads)   %8.3f ms  %8.1f GB/s\n", ms, 3.0 * N / ms / 1e6);
    }
  }
  if (what == "quantwg") {  // round 4: merged output pieces through a WAVES-wave workgroup, and padded row strides (KVQ_PAD_IN / KVQ_PAD_OUT tokens)
    const uint32_t pad_in = getenv("KVQ_PAD_IN") ? (uint32_t)atoll(getenv("KVQ_PAD_IN")) : 0u, pad_out = getenv("KVQ_PAD_OUT") ? (uint32_t)atoll(getenv("KVQ_PAD_OUT")) : 0u;
    const uint32_t padm = pad_in > pad_out ? pad_in : pad_out;
    const uint32_t Te = (uint32_t)((T - padm) / 32 * 32);  // tokens walked: rows of Te + pad tokens fit the T-token allocations
    const double n_e = (double)G * 8 * Te * 128;
    printf("# quantwg: pad_in=%u pad_out=%u tokens (row strides %lld / %lld B in, INT4 / INT8 %lld / %lld B out), %u tokens walked\n", pad_in, pad_out,
           (long long)(Te + pad_in) * 256, (long long)(Te + pad_in) * 256, (long long)(Te + pad_out) * 64, (long long)(Te + pad_out) * 128, Te);
#define RUN_WG(WV, BITS_)                                                                                          \
  {                                                                                                               \
    double best = 1e9, sum = 0;                                                                                   \
    for (int rep = 0; rep < 3; ++rep) {                                                                           \
      const double ms = tm.ms_per([&] { rotate(); rw_quant_tile_wg_k<WV, BITS_><<<dim3(Te / (4 * WV), (unsigned)G), WV * 64>>>((const u32x4*)in16, (u32x4*)out, Te, pad_in, pad_out); }, iters); \
      best = ms < best ? ms : best; sum += ms;                                                                    \
    }                                                                                                             \
    const double bpe = BITS_ == 4 ? 2.5 : 3.0;                                                                    \
    printf("calib quantwg INT%d waves=%d (row run %5d B)  best %8.3f ms  mean %8.3f ms  %8.1f GB/s  frac8T=%.3f\n", BITS_, WV, WV * 64 * BITS_, best, sum / 3, bpe * n_e / best / 1e6, bpe * n_e / best / 1e6 / 8000.0); \
  }
    RUN_WG(1, 4) RUN_WG(2, 4) RUN_WG(4, 4) RUN_WG(8, 4) RUN_WG(16, 4)
    RUN_WG(1, 8) RUN_WG(2, 8) RUN_WG(4, 8) RUN_WG(8, 8)
#undef RUN_WG
  }
  if (what == "quantpat") {  // the quantise kernels' loads + stores without arithmetic: one-wave tiles vs head-per-wave tiles
    const int64_t T_all = N / (8 * 128);           // tokens if the 1 GiB input were one [8][T][128] tensor
    const int64_t head_vec_in = T_all * 16, head_vec_out = T_all * 4;
    for (int rep = 0; rep < 3; ++rep) {
      double ms = tm.ms_per([&] { rotate(); rw_quant_tile_k<false><<<(unsigned)(T_all / 4), 64>>>((const u32x4*)in16, (u32x4*)out, head_vec_in, head_vec_out); }, iters);
      printf("calib quantpat one-wave tile (8 x 1 KiB in, 8 x 256 B out)        %8.3f ms  %8.1f GB/s (r+w, INT4 mix)\n", ms, 2.5 * N / ms / 1e6);
      ms = tm.ms_per([&] { rotate(); rw_quant_tile_k<true><<<(unsigned)(T_all / 32), 512>>>((const u32x4*)in16, (u32x4*)out, head_vec_in, head_vec_out); }, iters);
      printf("calib quantpat head-per-wave tile (8 KiB in, 2 KiB out per wave)  %8.3f ms  %8.1f GB/s (r+w, INT4 mix)\n", ms, 2.5 * N / ms / 1e6);
      ms = tm.ms_per([&] { rotate(); rw_quant_tile_real_k<<<dim3((unsigned)(T / 4), (unsigned)G), 64>>>((const u32x4*)in16, (u32x4*)out, (uint32_t)T); }, iters);
      printf("calib quantpat one-wave tile, the real tensors' strides (heads 4 MiB / 1 MiB apart)  %8.3f ms  %8.1f GB/s\n", ms, 2.5 * N / ms / 1e6);
      ms = tm.ms_per([&] { rotate(); rw_quant_tile_i8_k<true><<<dim3((unsigned)(T / 4), (unsigned)G), 64>>>((const u32x4*)in16, (u32x4*)out, (uint32_t)T); }, iters);
      printf("calib quantpat INT8 one-wave tile (8 x 1 KiB in, 8 x 512 B out, nt stores)  %8.3f ms  %8.1f GB/s\n", ms, 3.0 * N / ms / 1e6);
      ms = tm.ms_per([&] { rotate(); rw_quant_tile_i8_k<false><<<dim3((unsigned)(T / 4), (unsigned)G), 64>>>((const u32x4*)in16, (u32x4*)out, (uint32_t)T); }, iters);
      printf("calib quantpat INT8 one-wave tile (8 x 1 KiB in, 8 x 512 B out, plain stores)  %8.3f ms  %8.1f GB/s\n", ms, 3.0 * N / ms / 1e6);
#define RUN_NV(NV)                                                                                                 \
  ms = tm.ms_per([&] { rotate(); rw_quant_tile_k<false, NV><<<(unsigned)(T_all / 4), 64>>>((const u32x4*)in16, (u32x4*)out, head_vec_in, head_vec_out); }, iters); \
  printf("calib quantpat one-wave tile + %4d filler vector instructions       %8.3f ms  %8.1f GB/s (r+w, INT4 mix)\n", NV, ms, 2.5 * N / ms / 1e6);
      RUN_NV(128) RUN_NV(256) RUN_NV(512) RUN_NV(1024)
#undef RUN_NV
      {
        // pointer table: slot 0 = the data pointer, slot 1 = address of the next table (all the same table)
        static uintptr_t* d_tab[2] = {nullptr, nullptr};
        for (int b = 0; b < 2; ++b) {
          if (!d_tab[b]) HIP_OK(hipMalloc(&d_tab[b], 16));
          const uintptr_t h[2] = {(uintptr_t)in16s[b], (uintptr_t)d_tab[b]};
          HIP_OK(hipMemcpy(d_tab[b], h, 16, hipMemcpyHostToDevice));
        }
#define RUN_T2(L, C)                                                                                               \
  ms = tm.ms_per([&] { rotate(); rw_quant_tile2_k<L, C><<<(unsigned)(T_all / 4), 64>>>((const u32x4* const*)d_tab[rot % 2], (u32x4*)out, head_vec_in, head_vec_out); }, iters); \
  printf("calib quantpat one-wave tile, LDS-staged output=%d, %d dependent scalar loads first  %8.3f ms  %8.1f GB/s\n", (int)L, C, ms, 2.5 * N / ms / 1e6);
        RUN_T2(false, 1) RUN_T2(true, 1) RUN_T2(false, 3) RUN_T2(false, 5) RUN_T2(true, 4)
#undef RUN_T2
      }
    }
  }
  if (what == "poolpat") {  // one chunk per one-wave workgroup vs the shipped kernel's pattern
    const int64_t n_chunks = N * 2 / 16384;
    for (int rep = 0; rep < 3; ++rep) {
      double ms = tm.ms_per([&] { rotate(); read_chunk_rows_k<false><<<(unsigned)n_chunks, 64>>>((const u32x4*)in16, (uint32_t*)ws); }, iters);
      printf("calib chunkrows group-owns-16-rows  %8.3f ms  %8.1f GB/s (r, one 16 KiB chunk per wave, 4 x 256 B per load)\n", ms, 1.0 * N * 2 / ms / 1e6);
      ms = tm.ms_per([&] { rotate(); read_chunk_rows_k<true><<<(unsigned)n_chunks, 64>>>((const u32x4*)in16, (uint32_t*)ws); }, iters);
      printf("calib chunkrows row-quads           %8.3f ms  %8.1f GB/s (r, one 16 KiB chunk per wave, 1 KiB per load)\n", ms, 1.0 * N * 2 / ms / 1e6);
      const int grid = (int)((n_chunks * 16 + 255) / 256);
      ms = tm.ms_per([&] { rotate(); read_seg_k<16><<<grid, 256>>>((const u32x4*)in16, (uint32_t*)ws, n_chunks); }, iters);
      printf("calib readseg  batch=16 block=256   %8.3f ms  %8.1f GB/s (r, the shipped kernel's pattern)\n", ms, 1.0 * N * 2 / ms / 1e6);
    }
  }
  if (what == "fillchunk") {  // write-only ceiling, one-wave workgroups, one contiguous chunk each
    const int64_t bytes = N * 2;
#define RUN_FILL(VEC, NT)                                                                                         \
  {                                                                                                               \
    const unsigned grid = (unsigned)(bytes / ((int64_t)(VEC) * 16));                                              \
    double best = 1e9;                                                                                            \
    for (int rep = 0; rep < 3; ++rep) {                                                                           \
      const double ms = tm.ms_per([&] { rotate(); fill_chunk_k<VEC, NT><<<grid, 64>>>((u32x4*)out, 7u); }, iters);  \
      best = ms < best ? ms : best;                                                                               \
    }                                                                                                             \
    printf("calib fillchunk chunk=%6d B nt=%d  %8.3f ms  %8.1f GB/s (w)\n", (VEC) * 16, (int)(NT), best, 1.0 * bytes / best / 1e6); \
  }
    RUN_FILL(64, true) RUN_FILL(128, true) RUN_FILL(256, true) RUN_FILL(512, true) RUN_FILL(1024, true)
    RUN_FILL(64, false) RUN_FILL(128, false) RUN_FILL(256, false) RUN_FILL(512, false) RUN_FILL(1024, false)
#undef RUN_FILL
  }
  if (what == "fillaux") {  // 4 KiB per one-wave workgroup, every store cache policy
    const int64_t bytes = N * 2;
    const unsigned grid = (unsigned)(bytes / 4096);
#define RUN_AUX(A)                                                                                               \
  {                                                                                                               \
    double best = 1e9;                                                                                            \
    for (int rep = 0; rep < 3; ++rep) {                                                                           \
      const double ms = tm.ms_per([&] { rotate(); fill_chunk_aux_k<A><<<grid, 64>>>((u32x4*)out, 7u); }, iters);  \
      best = ms < best ? ms : best;                                                                               \
    }                                                                                                             \
    printf("calib fillaux aux=%2d (sc0=%d nt=%d sc1=%d)  %8.3f ms  %8.1f GB/s (w)\n", A, (A) & 1, ((A) >> 1) & 1, ((A) >> 4) & 1, best, 1.0 * bytes / best / 1e6); \
  }
    RUN_AUX(0) RUN_AUX(1) RUN_AUX(2) RUN_AUX(3) RUN_AUX(16) RUN_AUX(17) RUN_AUX(18) RUN_AUX(19)
#undef RUN_AUX
  }
  if (what == "segread") {  // S strided segments per one-wave workgroup (the quantise tile) vs one contiguous chunk
    const int64_t bytes = N * 2;
#define RUN_SEG(S, LVEC)                                                                                          \
  {                                                                                                               \
    const int64_t seg_stride_vec = bytes / 16 / (S);                                                              \
    const unsigned grid = (unsigned)(seg_stride_vec / (LVEC));                                                    \
    double best = 1e9;                                                                                            \
    for (int rep = 0; rep < 3; ++rep) {                                                                           \
      const double ms = tm.ms_per([&] { rotate(); read_segments_k<S, LVEC><<<grid, 64>>>((const u32x4*)in16, (uint32_t*)ws, seg_stride_vec); }, iters); \
      best = ms < best ? ms : best;                                                                               \
    }                                                                                                             \
    printf("calib segread S=%2d L=%6d B (%6d B per workgroup)  %8.3f ms  %8.1f GB/s (r)\n", S, (LVEC) * 16, (S) * (LVEC) * 16, best, 1.0 * bytes / best / 1e6); \
  }
    RUN_SEG(1, 256) RUN_SEG(1, 512) RUN_SEG(1, 1024)
    RUN_SEG(2, 128) RUN_SEG(2, 256) RUN_SEG(4, 64) RUN_SEG(4, 128) RUN_SEG(4, 256)
    RUN_SEG(8, 64) RUN_SEG(8, 128) RUN_SEG(8, 256) RUN_SEG(16, 64) RUN_SEG(16, 128)
#undef RUN_SEG
  }
  if (what == "readpat") {  // read patterns of the chunk mean-pool kernel, no arithmetic
    const int64_t n_chunks = N * 2 / 16384;
    const int grid = (int)((n_chunks * 16 + 255) / 256);
    const int grid64 = (int)(n_chunks / 4);
    const int64_t n16 = N * 2 / 16;
    for (int rep = 0; rep < 3; ++rep) {
      double ms = tm.ms_per([&] { rotate(); read_seg_k<16><<<grid, 256>>>((const u32x4*)in16, (uint32_t*)ws, n_chunks); }, iters);
      printf("calib readseg  batch=16 block=256 %8.3f ms  %8.1f GB/s (r, 4 x 256 B segments per wave load)\n", ms, 1.0 * N * 2 / ms / 1e6);
      ms = tm.ms_per([&] { rotate(); read_seg_rows_k<8><<<grid64, 64>>>((const u32x4*)in16, (uint32_t*)ws, n_chunks); }, iters);
      printf("calib readrows batch=8  block=64  %8.3f ms  %8.1f GB/s (r, 1 KiB contiguous per wave load)\n", ms, 1.0 * N * 2 / ms / 1e6);
      ms = tm.ms_per([&] { rotate(); read_seg_rows_k<16><<<grid64, 64>>>((const u32x4*)in16, (uint32_t*)ws, n_chunks); }, iters);
      printf("calib readrows batch=16 block=64  %8.3f ms  %8.1f GB/s (r, 1 KiB contiguous per wave load)\n", ms, 1.0 * N * 2 / ms / 1e6);
      ms = tm.ms_per([&] { rotate(); read_seg_rows_k<32><<<grid64, 64>>>((const u32x4*)in16, (uint32_t*)ws, n_chunks); }, iters);
      printf("calib readrows batch=32 block=64  %8.3f ms  %8.1f GB/s (r, 1 KiB contiguous per wave load)\n", ms, 1.0 * N * 2 / ms / 1e6);
      ms = tm.ms_per([&] { rotate(); read16_k<<<4096, 256>>>((const u32x4*)in16, (uint32_t*)ws, n16); }, iters);
      printf("calib read16   grid=4096  %8.3f ms  %8.1f GB/s (r)\n", ms, 1.0 * N * 2 / ms / 1e6);
    }
  }
  if (what == "copy" || what == "all") {
    const int64_t n16 = N * 2 / 16;  // 1 GiB
    for (int grid : {2048, 4096, 16384, 65536}) {
      double ms = tm.ms_per([&] { rotate(); copy16_k<<<grid, 256>>>((const u32x4*)in16, (u32x4*)out, n16); }, iters);
      printf("calib copy16   grid=%6d  %8.3f ms  %8.1f GB/s (r+w)\n", grid, ms, 2.0 * N * 2 / ms / 1e6);
    }
    for (int grid : {2048, 4096, 16384, 65536}) {
      double ms = tm.ms_per([&] { rotate(); fill16_k<<<grid, 256>>>((u32x4*)out, n16, 7u); }, iters);
      printf("calib fill16   grid=%6d  %8.3f ms  %8.1f GB/s (w)\n", grid, ms, 1.0 * N * 2 / ms / 1e6);
    }
    {
      struct Ctx { decltype(rotate)* r; } ctx{&rotate};
      auto rot = [](void* c) { (*static_cast<Ctx*>(c)->r)(); };
#define RUN_TILE(BLOCK, U, NT)                                                                              \
  {                                                                                                         \
    const int64_t per = (int64_t)BLOCK * U;                                                                 \
    const unsigned grid = (unsigned)((n16 + per - 1) / per);                                                \
    double ms = tm.ms_per([&] { rotate(); copy16_tile_k<BLOCK, U, NT><<<grid, BLOCK>>>((const u32x4*)in16, (u32x4*)out, n16); }, iters); \
    printf("calib copytile block=%4d U=%d nt=%d  %8.3f ms  %8.1f GB/s (r+w)\n", BLOCK, U, (int)NT, ms, 2.0 * N * 2 / ms / 1e6); \
  }
      (void)rot; (void)ctx;
      RUN_TILE(64, 1, false) RUN_TILE(64, 2, false) RUN_TILE(64, 4, false) RUN_TILE(128, 1, false) RUN_TILE(128, 2, false)
      RUN_TILE(64, 4, true) RUN_TILE(128, 2, true) RUN_TILE(256, 1, true)
      RUN_TILE(256, 1, false) RUN_TILE(256, 2, false) RUN_TILE(256, 4, false) RUN_TILE(256, 8, false)
      RUN_TILE(512, 4, false) RUN_TILE(1024, 4, false) RUN_TILE(1024, 1, false)
      RUN_TILE(256, 4, true) RUN_TILE(256, 8, true) RUN_TILE(512, 4, true) RUN_TILE(1024, 2, true)
#undef RUN_TILE
    }
    for (int grid : {4096, 65536}) {
      double ms = tm.ms_per([&] { rotate(); fill16_nt_k<<<grid, 256>>>((u32x4*)out, n16, 7u); }, iters);
      printf("calib fill16nt grid=%6d  %8.3f ms  %8.1f GB/s (w)\n", grid, ms, 1.0 * N * 2 / ms / 1e6);
    }
    for (int grid : {4096, 65536}) {
      double ms = tm.ms_per([&] { rotate(); copy16_nt_k<<<grid, 256>>>((const u32x4*)in16, (u32x4*)out, n16); }, iters);
      printf("calib copy16nt grid=%6d  %8.3f ms  %8.1f GB/s (r+w)\n", grid, ms, 2.0 * N * 2 / ms / 1e6);
    }
    for (int nt = 0; nt < 2; ++nt)
      for (int grid : {4096, 65536, 262144}) {
        double ms = tm.ms_per([&] { rotate(); expand4_k<<<grid, 256>>>((const uint32_t*)q4, (u32x4*)out, n16, nt); }, iters);
        printf("calib expand4 nt=%d grid=%6d  %8.3f ms  %8.1f GB/s (0.25r+1w: the INT4 dequant mix)\n", nt, grid, ms, 2.5 * N / ms / 1e6);
      }
    {
      const int64_t n_chunks = N * 2 / 16384;
      const int grid = (int)((n_chunks * 16 + 255) / 256);
      double ms = tm.ms_per([&] { rotate(); read_seg_k<8><<<grid, 256>>>((const u32x4*)in16, (uint32_t*)ws, n_chunks); }, iters);
      printf("calib readseg  batch=8   %8.3f ms  %8.1f GB/s (r, 4 x 256 B segments per wave load)\n", ms, 1.0 * N * 2 / ms / 1e6);
      ms = tm.ms_per([&] { rotate(); read_seg_k<16><<<grid, 256>>>((const u32x4*)in16, (uint32_t*)ws, n_chunks); }, iters);
      printf("calib readseg  batch=16  %8.3f ms  %8.1f GB/s (r, 4 x 256 B segments per wave load)\n", ms, 1.0 * N * 2 / ms / 1e6);
      ms = tm.ms_per([&] { rotate(); read_seg_k<32><<<grid, 256>>>((const u32x4*)in16, (uint32_t*)ws, n_chunks); }, iters);
      printf("calib readseg  batch=32  %8.3f ms  %8.1f GB/s (r, 4 x 256 B segments per wave load)\n", ms, 1.0 * N * 2 / ms / 1e6);
      const int grid64 = (int)(n_chunks / 4);
      ms = tm.ms_per([&] { rotate(); read_seg_rows_k<16><<<grid64, 64>>>((const u32x4*)in16, (uint32_t*)ws, n_chunks); }, iters);
      printf("calib readrows batch=16 block=64  %8.3f ms  %8.1f GB/s (r, 1 KiB contiguous per wave load, 4 chunks per wave)\n", ms, 1.0 * N * 2 / ms / 1e6);
      ms = tm.ms_per([&] { rotate(); read_seg_rows_k<32><<<grid64, 64>>>((const u32x4*)in16, (uint32_t*)ws, n_chunks); }, iters);
      printf("calib readrows batch=32 block=64  %8.3f ms  %8.1f GB/s (r, 1 KiB contiguous per wave load, 4 chunks per wave)\n", ms, 1.0 * N * 2 / ms / 1e6);
      ms = tm.ms_per([&] { rotate(); read_seg_rows_k<8><<<grid64, 64>>>((const u32x4*)in16, (uint32_t*)ws, n_chunks); }, iters);
      printf("calib readrows batch=8  block=64  %8.3f ms  %8.1f GB/s (r, 1 KiB contiguous per wave load, 4 chunks per wave)\n", ms, 1.0 * N * 2 / ms / 1e6);
    }
    for (int grid : {2048, 4096, 16384}) {
      double ms = tm.ms_per([&] { rotate(); read16_k<<<grid, 256>>>((const u32x4*)in16, (uint32_t*)ws, n16); }, iters);
      printf("calib read16   grid=%6d  %8.3f ms  %8.1f GB/s (r)\n", grid, ms, 1.0 * N * 2 / ms / 1e6);
    }
  }

  auto run_dequant = [&](int bits) {
    const double bytes = bits == 4 ? N * 2.5 : N * 3.0;
    double ms = tm.ms_per(
        [&] {
          rotate();
          if (bits == 4)
            KVQ_OK(kvq_dequant_i4_tokens((const uint8_t*)q4, &s_half, scales, T, out, &s_full, KVQ_F16, &dims, 0));
          else
            KVQ_OK(kvq_dequant_i8_tokens((const int8_t*)q8, &s_full, scales, T, out, &s_full, KVQ_F16, &dims, 0));
        },
        iters);
    printf("dequant_i%d  %8.3f ms  %8.1f GB/s  frac8T=%.3f\n", bits, ms, bytes / ms / 1e6, bytes / ms / 1e6 / 8000.0);
  };
  if (what == "dequant4" || what == "all") run_dequant(4);
  if (what == "dequant8" || what == "all") run_dequant(8);

  if (what == "mixed" || what == "all") {  // one decode step's two dequantise calls back to back (INT8 K, INT4 V)
    hipEvent_t e0, e1, e2;
    HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1)); HIP_OK(hipEventCreate(&e2));
    double t8 = 0, t4 = 0;
    for (int it = 0; it < iters + 3; ++it) {
      rotate();
      HIP_OK(hipEventRecord(e0, 0));
      KVQ_OK(kvq_dequant_i8_tokens((const int8_t*)q8, &s_full, scales, T, outs[0], &s_full, KVQ_F16, &dims, 0));
      HIP_OK(hipEventRecord(e1, 0));
      KVQ_OK(kvq_dequant_i4_tokens((const uint8_t*)q4, &s_half, scales, T, outs[1], &s_full, KVQ_F16, &dims, 0));
      HIP_OK(hipEventRecord(e2, 0));
      HIP_OK(hipEventSynchronize(e2));
      float a = 0, b = 0;
      HIP_OK(hipEventElapsedTime(&a, e0, e1)); HIP_OK(hipEventElapsedTime(&b, e1, e2));
      if (it >= 3) { t8 += a; t4 += b; }
    }
    printf("mixed step  i8 %7.3f ms %7.1f GB/s | i4 %7.3f ms %7.1f GB/s | step %7.1f GB/s\n", t8 / iters,
           N * 3.0 / (t8 / iters) / 1e6, t4 / iters, N * 2.5 / (t4 / iters) / 1e6, N * 5.5 / ((t8 + t4) / iters) / 1e6);
  }

  auto run_quant = [&](int bits) {
    const double bytes = bits == 4 ? N * 2.5 : N * 3.0;
    for (int two_pass = 0; two_pass < (what == "qblock" ? 1 : 2); ++two_pass) {
      KVQ_OK(kvq_set_tunable("quant_force_two_pass", two_pass));
      double ms = tm.ms_per(
          [&] {
            rotate();
            if (bits == 4)
              KVQ_OK(kvq_quant_i4_tokens(in16, nullptr, &s_full, KVQ_F16, (uint8_t*)q4, &s_half, scales, T, ws, 1e-8f, &dims, 0));
            else
              KVQ_OK(kvq_quant_i8_tokens(in16, nullptr, &s_full, KVQ_F16, (int8_t*)q8, &s_full, scales, T, ws, 1e-8f, &dims, 0));
          },
          two_pass ? 3 : iters, 1);
      printf("quant_i%d  two_pass=%d  %8.3f ms  %8.1f GB/s (algorithmic single-pass bytes)  frac8T=%.3f\n", bits, two_pass,
             ms, bytes / ms / 1e6, bytes / ms / 1e6 / 8000.0);
    }
    KVQ_OK(kvq_set_tunable("quant_force_two_pass", 0));
  };
  if (what == "qblock") {  // the general quantise kernel: 256-thread workgroups against one-wave tiles
    for (int blk : {256, 64, 256, 64}) {
      KVQ_OK(kvq_set_tunable("quant_block", blk));
      printf("quant_block=%d\n", blk);
      run_quant(4);
      run_quant(8);
    }
    KVQ_OK(kvq_set_tunable("quant_block", 64));
  }
  if (what == "quant4" || what == "all") run_quant(4);
  if (what == "quant8" || what == "all") run_quant(8);

  if (what == "pool" || what == "all") {
    // chunk summary of the fp16 KV: chunk 64, keep_last 256 (CacheConfig defaults)
    const int64_t Tout = kvq_chunk_summary_len(T, 64, 256);
    kvq_strides_t s_out = {B * H * Tout * D, H * Tout * D, Tout * D, D};
    const double bytes = 2.0 * G * B * H * D * (T + Tout);
    double ms = tm.ms_per([&] { rotate(); KVQ_OK(kvq_chunk_meanpool(in16, nullptr, &s_full, out, &s_out, KVQ_F16, 64, 256, &dims, 0)); }, iters);
    printf("chunk_meanpool T=%lld->%lld  %8.3f ms  %8.1f GB/s  frac8T=%.3f\n", (long long)T, (long long)Tout, ms, bytes / ms / 1e6,
           bytes / ms / 1e6 / 8000.0);
  }
  if (what == "window" || what == "all") {
    for (int64_t W : {(int64_t)256, (int64_t)8192}) {
      kvq_strides_t s_out = {B * H * W * D, H * W * D, W * D, D};
      const double bytes = 4.0 * G * B * H * W * D;
      double ms = tm.ms_per([&] { rotate(); KVQ_OK(kvq_window_compact(in16, nullptr, &s_full, out, &s_out, 2, W, &dims, 0)); }, iters);
      printf("window_compact W=%lld  %8.3f ms  %8.1f GB/s  frac8T=%.3f\n", (long long)W, ms, bytes / ms / 1e6,
             bytes / ms / 1e6 / 8000.0);
    }
  }
  HIP_OK(hipDeviceSynchronize());
  printf("# done\n");
  return 0;
}

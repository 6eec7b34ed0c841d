// ring.inc — part of kvq_attn.hip (one translation unit, included in this order): decode_attn_lds_mfma_k: the LDS-staged (LDS-DMA ring) streaming kernel — what ships for large batches, head_dim 128 and 64
// ---------------------------------------------------------------------------- LDS-staged streaming variant
// A register-staged streaming kernel (AttnStream::issue) asks HBM for its rows in MFMA-operand shape: a K load instruction touches sixteen rows,
// 64 B of each (lane (x, g): 16 B at row x, byte 16 g), a V load four rows — half-line and sub-line pieces whose
// address processing (TA) and DRAM efficiency cap the loads-only build of that kernel at 5.6 TB/s where contiguous
// reads reach 7.0 (profiles/r02ab, r02ae). Here a 64-token tile — one CONTIGUOUS run of the store for a (batch row,
// kv head): 8 KiB of INT8 keys, 4 KiB of INT4 values — travels as whole 1 KiB wave requests straight into LDS
// (`buffer_load_dwordx4 ... lds`: LDS-DMA, no VGPRs, range-checked by the descriptor like every row load in this file),
// NB - 1 tiles ahead of the one being reduced in a ring of NB LDS slots, and the MFMA operand fragments are read from
// LDS in exactly the register layout AttnStream::consume already takes (same arithmetic, same operand order: results
// are bit-identical to the streaming kernel's). In flight per wave: (NB - 1) x 12.5 KiB held by LDS instead of
// registers; the K image is XOR-swizzled on the SOURCE address (LDS-DMA writes lane-linear) so that the ds_read_b128
// fragment reads are bank-conflict free: slot s of row r holds 16-byte chunk s ^ f(r),
//   INT8 keys (8 chunks per row): f(r) = (r >> 1) & 7        INT4 keys (4 chunks per row): f(r) = r & 8 ? 3 : 0
// (derivation: the four 16-lane groups of ds_read_b128, MI355X_MICROARCH.md LDS table). The V rows are read as the
// streaming kernel reads them from memory (4 or 8 bytes per lane; rows r and r + 4 share a bank half: 2-way, on an
// LDS that is far from busy). Completion: every request of a tile is an LDS-DMA, so `s_waitcnt vmcnt(OPS x (NB-1))`
// is "tile k has landed" (loads retire in order); tiles past the wave's last are requested with an empty descriptor
// (nothing is read) so that the count is the same in every iteration.
template <int KCPR>  // 16-byte chunks per stored key row: 8 (128 B: INT8 at head_dim 128) or 4 (64 B: INT4 at 128, INT8 at 64)
__device__ inline uint32_t k_swizzle(uint32_t row) {
  static_assert(KCPR == 8 || KCPR == 4, "key rows of 128 or 64 bytes");
  if constexpr (KCPR == 8) return (row >> 1) & 7u;
  else return (row & 8u) ? 3u : 0u;
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {  // s_waitcnt vmcnt(N) only (expcnt / lgkmcnt fields at their maxima)
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}

// MFMA operand fragments of one tile out of its LDS image (K rows swizzled as k_swizzle says, V rows plain), in
// AttnStream::Raw's register layout: lane (x, g) takes the 16 K bytes of row 16 i + x at chunk 4 c + g, and the V bytes
// of its eight token rows per 32-token step.
template <int KBITS, int VBITS, int TC, bool KI8, class RAW, int HD = 128>
__device__ __forceinline__ void read_fragments(const uint8_t* img, RAW& r) {  // RAW: AttnStream<...>::Raw of any TG
  typedef AttnStream<KBITS, VBITS, TC, HD, KI8, false> ST;
  constexpr int NT = ST::NT, NS = ST::NS, NL = ST::NL, VB = ST::VB;
  constexpr int KROW = HD * KBITS / 8, VROW = HD * VBITS / 8;
  const uint32_t lane = threadIdx.x & 63u, x = lane & 15u, g = lane >> 4;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const uint32_t row = 16u * i + x;
#pragma unroll
    for (int c = 0; c < NL; ++c) {
      const u32x4 w = *reinterpret_cast<const u32x4*>(img + row * KROW + (((4u * c + g) ^ k_swizzle<KROW / 16>(row)) << 4));
#pragma unroll
      for (int j = 0; j < 4; ++j) r.k[i][c][j] = w[j];
    }
  }
  const uint8_t* vimg = img + TC * KROW;
#pragma unroll
  for (int sidx = 0; sidx < NS; ++sidx) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t row = 32u * sidx + 16u * (j >> 2) + (j & 3) + 4u * g;
      if constexpr (VB == 8) {
        const u32x2 w = *reinterpret_cast<const u32x2*>(vimg + row * VROW + 8u * x);
        r.v[sidx][j][0] = w[0];
        r.v[sidx][j][VB == 8 ? 1 : 0] = w[1];
      } else if constexpr (VB == 4) {
        r.v[sidx][j][0] = *reinterpret_cast<const uint32_t*>(vimg + row * VROW + 4u * x);
      } else {  // head_dim 64, INT4 values: 2 bytes (4 elements) per lane and row
        static_assert(VB == 2, "V bytes per lane and row");
        r.v[sidx][j][0] = (uint32_t)*reinterpret_cast<const uint16_t*>(vimg + row * VROW + 2u * x);
      }
    }
  }
}

// decode_attn_lds_mfma_k and decode_attn_lds_mfma_padded_k: one kernel text (ring_kernel.inc), compiled twice; a third time as
// decode_attn_lds_mfma_mod_k, the soft-capped form
#define KVQ_RING_PADDED 0
#include "ring_kernel.inc"
#undef KVQ_RING_PADDED
#define KVQ_RING_PADDED 1
#include "ring_kernel.inc"
#undef KVQ_RING_PADDED
#define KVQ_RING_PADDED 2
#include "ring_kernel.inc"
#undef KVQ_RING_PADDED

// merge.inc — part of kvq_attn.hip (one translation unit, included in this order): the merge kernels (chained, one-round-trip, one wave per head) + the new token's quantise-append
constexpr int kAttnMfmaTC = 128;

constexpr int kAttnMaxSplit = 4096;  // merge: LDS weights + 16 (m, l) pairs per thread; T <= 512 Ki tokens at 128 per split

// A new-token slice past the register path (more than 8,192 elements: batch > 8 at 8 kv heads x 128). The generic routine
// walked it with ONE workgroup, element by element, twice: 40 us at batch 16 and 158 us at batch 64 on top of a 17 / 43 us
// attention (profiles/r04ac_decode_step_by_batch.jsonl; with this routine: + 3 / + 10 us, the merge launch 7.9 / 8.9 us under
// rocprofv3 against 4.0 / 4.9 without an append) — every layer of every decode step. Here the slice is cut into
// a.nparts pieces (host: one per 8,192 elements), one workgroup each: EVERY workgroup takes the abs-max of the WHOLE slice
// (16-byte loads, 16 in flight per thread; 128 KiB at most, the same lines for all of them) — so nothing crosses workgroups —
// and quantises only its own piece, with the generic routine's expressions per element (IEEE divide, round-half-even):
// the same bytes and the same scale. Host-checked preconditions: D % 8 == 0, 16-byte aligned rows of x, store rows aligned
// to the 8 / 4 bytes a vector's codes take.
template <int IDT>
__device__ inline void quant_new_token_parts(const NewTokenArgs& a, const uint32_t w, const uint32_t part, float* s_red) {
  constexpr int UN = 32;  // 65,536 elements (the host's bound) = 32 vectors per thread: every load of the abs-max pass is in flight at once
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  const uint32_t tid = threadIdx.x;
  const uint32_t DV = a.D >> 3, nvec = a.B * a.H * DV;
  const uint16_t* x = reinterpret_cast<const uint16_t*>(a.x[w]);
  auto src = [&](const uint32_t v, uint32_t& b, uint32_t& h, uint32_t& piece) -> const u32x4* {
    const uint32_t row = v / DV;
    piece = v - row * DV;
    b = row / a.H;
    h = row - b * a.H;
    return reinterpret_cast<const u32x4*>(x + (int64_t)b * a.xs_b[w] + (int64_t)h * a.xs_h[w] + piece * 8u);
  };
  auto elem = [](const u32x4& r, const int e) -> float { return Elem<IDT>::widen((uint16_t)((r[e >> 1] >> (16 * (e & 1))) & 0xFFFFu)); };
  // this workgroup's own piece first: its (at most OWN) vectors per thread are requested together with the whole slice and stay in
  // registers across the reduction, so the routine is ONE memory round trip (a second pass that re-read them measured 8.5 us per
  // launch at batch 16 where the merge workgroups of the same launch take 4)
  constexpr int OWN = 4;  // chunk <= OWN * kAttnBlock vectors: the host cuts one piece per 8,192 elements
  const uint32_t chunk = (nvec + a.nparts - 1u) / a.nparts;
  const uint32_t lo = part * chunk, hi = lo + chunk < nvec ? lo + chunk : nvec;
  u32x4 own[OWN];
  uint32_t ob[OWN], oh[OWN], op[OWN];
#pragma unroll
  for (int k = 0; k < OWN; ++k) {
    const uint32_t v = lo + tid + (uint32_t)(k * kAttnBlock);
    own[k] = u32x4{0u, 0u, 0u, 0u};
    ob[k] = oh[k] = op[k] = 0u;
    if (v < hi) own[k] = *src(v, ob[k], oh[k], op[k]);
  }
  // abs-max on the bit patterns: |x| of a half / bfloat16 is its low 15 bits, and those order like the values (finite inputs,
  // as everywhere in this library): two elements per packed unsigned max, one conversion at the end
  u16x2 mb = {0, 0};
  // the slice walk advances kAttnBlock vectors = RPP rows per step: (b, h) move by a uniform (quotient, remainder) of RPP / H
  // instead of two integer divisions per vector (72 divisions per thread were most of this routine's time)
  const uint32_t dvsh = DV == 16u ? 4u : 3u;  // host: head_dim 128 or 64
  const uint32_t RPP = (uint32_t)kAttnBlock >> dvsh, qstep = RPP / a.H, rstep = RPP - qstep * a.H;
  const uint32_t wpiece = tid & (DV - 1u);
  uint32_t wb = (tid >> dvsh) / a.H, wh = (tid >> dvsh) - wb * a.H;
  for (uint32_t v0 = tid; v0 < nvec; v0 += (uint32_t)(kAttnBlock * UN)) {
    u32x4 r[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const uint32_t v = v0 + (uint32_t)(u * kAttnBlock);
      r[u] = u32x4{0u, 0u, 0u, 0u};
      if (v < nvec) r[u] = *reinterpret_cast<const u32x4*>(x + (int64_t)wb * a.xs_b[w] + (int64_t)wh * a.xs_h[w] + wpiece * 8u);
      wb += qstep;
      wh += rstep;
      if (wh >= a.H) {
        wh -= a.H;
        ++wb;
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t absb = r[u][c] & 0x7FFF7FFFu;
        u16x2 pair;
        __builtin_memcpy(&pair, &absb, 4);
        mb = __builtin_elementwise_max(mb, pair);
      }
  }
  float m = Elem<IDT>::widen(mb[0] > mb[1] ? mb[0] : mb[1]);
  m = block_max_nonneg(m, s_red);
  auto codes8 = [&](const u32x4& r, const float s32) -> u32x2 {
    u32x2 o = {0u, 0u};
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e >> 2] |= ((uint32_t)(uint8_t)(int8_t)quant1<8>(elem(r, e), s32)) << (8 * (e & 3));
    return o;
  };
  auto codes4 = [&](const u32x4& r, const float s32) -> uint32_t {
    uint32_t o = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // even index -> high nibble
      const int h4 = quant1<4>(elem(r, 2 * j), s32) + 8, l4 = quant1<4>(elem(r, 2 * j + 1), s32) + 8;
      o |= (uint32_t)(((h4 & 0xF) << 4) | (l4 & 0xF)) << (8 * j);
    }
    return o;
  };
  if (a.bits[w] == 8) {
    const float s32 = fmaxf(m / QRange<8>::qmax, a.eps);
    if (tid == 0u && part == 0u) *a.scale[w] = Elem<IDT>::round_trip(s32);
#pragma unroll
    for (int k = 0; k < OWN; ++k)
      if (lo + tid + (uint32_t)(k * kAttnBlock) < hi)
        *reinterpret_cast<u32x2*>(a.q[w] + (int64_t)ob[k] * a.qs_b[w] + (int64_t)oh[k] * a.qs_h[w] + op[k] * 8u) = codes8(own[k], s32);
    for (uint32_t v = lo + tid + (uint32_t)(OWN * kAttnBlock); v < hi; v += kAttnBlock) {  // (pieces the host never cuts: past OWN vectors per thread)
      uint32_t b, h, piece;
      const u32x4 r = *src(v, b, h, piece);
      *reinterpret_cast<u32x2*>(a.q[w] + (int64_t)b * a.qs_b[w] + (int64_t)h * a.qs_h[w] + piece * 8u) = codes8(r, s32);
    }
  } else {
    const float s32 = fmaxf(m / QRange<4>::qmax, a.eps);
    if (tid == 0u && part == 0u) *a.scale[w] = Elem<IDT>::round_trip(s32);
#pragma unroll
    for (int k = 0; k < OWN; ++k)
      if (lo + tid + (uint32_t)(k * kAttnBlock) < hi)
        *reinterpret_cast<uint32_t*>(a.q[w] + (int64_t)ob[k] * a.qs_b[w] + (int64_t)oh[k] * a.qs_h[w] + op[k] * 4u) = codes4(own[k], s32);
    for (uint32_t v = lo + tid + (uint32_t)(OWN * kAttnBlock); v < hi; v += kAttnBlock) {
      uint32_t b, h, piece;
      const u32x4 r = *src(v, b, h, piece);
      *reinterpret_cast<uint32_t*>(a.q[w] + (int64_t)b * a.qs_b[w] + (int64_t)h * a.qs_h[w] + piece * 4u) = codes4(r, s32);
    }
  }
}

// One workgroup per (query head, batch row): log-sum-exp merge of the splits and of the exact new
// token. Split weights are computed once (one split per thread) and kept in LDS; the weighted sum
// runs 256 / D split groups wide with independent loads.
// With fuse_quant, two extra workgroups (blockIdx.x = Hq, Hq + 1 of batch row 0) quantise the new
// token's K / V into slot T of the stores (quant_new_token_block): nothing in this launch reads that
// slot, and the partial kernel that read [0, T) has finished, so a decode step is two launches.
__global__ __launch_bounds__(kAttnBlock) void decode_attn_merge_k(const AttnArgs a, const NewTokenArgs nt, const int fuse_quant) {
  __shared__ float s_red[kAttnBlock / kWave];
  if (blockIdx.x >= a.Hq) {  // new-token workgroups: (K | V) x pieces (one piece unless nt.nparts > 1)
    if (fuse_quant && blockIdx.y == 0u) {
      const uint32_t idx = blockIdx.x - a.Hq, wkv = idx & 1u, part = idx >> 1;
      NewTokenArgs slot = nt;
      if (a.t_dev) {  // the host passed slot 0; the real slot is the device-side T
        const int64_t T = (int64_t)live_tokens(a);
#pragma unroll
        for (int w = 0; w < 2; ++w) {
          slot.q[w] += T * nt.qs_t[w];
          slot.scale[w] += T;
        }
      }
      if (nt.nparts > 1u) {
        if (a.dtype == KVQ_F16) quant_new_token_parts<KVQ_F16>(slot, wkv, part, s_red);
        else quant_new_token_parts<KVQ_BF16>(slot, wkv, part, s_red);
      } else if (a.dtype == KVQ_F16) quant_new_token_block<KVQ_F16>(slot, wkv, s_red);
      else quant_new_token_block<KVQ_BF16>(slot, wkv, s_red);
    }
    return;
  }
  __shared__ float s_wt[kAttnMaxSplit];
  __shared__ __attribute__((aligned(16))) float s_out[kAttnBlock * 4];
  const uint32_t tid = threadIdx.x;
  const uint32_t hq = blockIdx.x, b = blockIdx.y;
  const uint32_t hk = hq / a.nq;
  const bool has_new = a.kn != nullptr;
  const uint32_t wave = tid >> 6, lane = tid & 63u;
  auto block_reduce = [&](float v, bool is_max) -> float {
    v = is_max ? wave_fmax(v) : wave_fsum(v);
    __syncthreads();  // s_red free again
    if (lane == 0u) s_red[wave] = v;
    __syncthreads();
    return is_max ? fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3])) : (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
  };
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  float s_tok = -INFINITY;
  if (has_new) {
    float part = 0.0f;
    for (uint32_t d = tid; d < a.D; d += kAttnBlock)
      part += load_elem(a.q, (int64_t)b * a.q_sb + (int64_t)hq * a.q_sh + d, a.dtype) *
              load_elem(a.kn, (int64_t)b * a.kn_sb + (int64_t)hk * a.kn_sh + d, a.dtype);
    s_tok = block_reduce(part, false) * a.sm_scale;
  }
  const float* ml = a.ws + ((int64_t)b * a.Hq + hq) * a.nsplit * 2;
  const float* accb = a.ws + a.acc_off + ((int64_t)b * a.Hq + hq) * a.nsplit * a.D;
  // a.nsplit is the row stride of the partials; with a device-side T only the first ceil(T / TS) are live
  uint32_t ns = a.nsplit;
  if (a.t_dev) {  // (kept out of the host-count path: evaluated there it cost the batch-1 call 0.7 us)
    const uint32_t t = live_tokens(a), lt = t - window_lo(a, t), ns_ts = live_split_tokens(a, lt);
    ns = (lt + ns_ts - 1u) / ns_ts;
  }
  // this thread's splits: tid, tid + 256, ...; (m, l) is read twice (second time from cache) rather
  // than kept in a register array sized for kAttnMaxSplit
  float m_max = s_tok;
  for (uint32_t s = tid; s < ns; s += kAttnBlock) m_max = fmaxf(m_max, ml[2 * s]);
  const float M = block_reduce(m_max, true);
  float lsum = 0.0f;
  for (uint32_t s = tid; s < ns; s += kAttnBlock) {
    const float w = __expf(ml[2 * s] - M);
    s_wt[s] = w;
    lsum += ml[2 * s + 1] * w;
  }
  const float w_new = has_new ? __expf(s_tok - M) : 0.0f;
  const float L = block_reduce(lsum, false) + w_new;  // the barriers inside also publish s_wt
  const float inv = 1.0f / L;
  // weighted sum, 16 bytes per lane: thread = (split group g, 4 elements at d4); 1024 / D groups.
  // (Requesting the first 8 rows + the new-token operands before the reductions measured slower:
  // 7.6 vs 5.1 us at 128 splits.)
  const uint32_t dv = a.D >> 2;
  const uint32_t groups = kAttnBlock / dv;  // 32, 16, 8 or 4
  const uint32_t g = tid / dv, d4 = tid - g * dv;
  f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
  {
    const f32x4* src = reinterpret_cast<const f32x4*>(accb) + d4;
    uint32_t s = g;
    for (; s + 7u * groups < ns; s += 8u * groups) {  // 8 independent loads in flight: at batch 1 the merge is pure latency
      f32x4 x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = src[(int64_t)(s + (uint32_t)u * groups) * dv];
#pragma unroll
      for (int u = 0; u < 8; ++u) o += x[u] * s_wt[s + (uint32_t)u * groups];
    }
    for (; s + 3u * groups < ns; s += 4u * groups) {  // 4 independent loads in flight
      const f32x4 x0 = src[(int64_t)s * dv];
      const f32x4 x1 = src[(int64_t)(s + groups) * dv];
      const f32x4 x2 = src[(int64_t)(s + 2u * groups) * dv];
      const f32x4 x3 = src[(int64_t)(s + 3u * groups) * dv];
      o += x0 * s_wt[s] + x1 * s_wt[s + groups] + x2 * s_wt[s + 2u * groups] + x3 * s_wt[s + 3u * groups];
    }
    for (; s < ns; s += groups) o += src[(int64_t)s * dv] * s_wt[s];
  }
  *reinterpret_cast<f32x4*>(&s_out[tid * 4]) = o;  // [g][d]
  __syncthreads();
  if (tid < a.D) {
    float t = 0.0f;
    for (uint32_t k = 0; k < groups; ++k) t += s_out[k * a.D + tid];
    if (has_new) t = fmaf(w_new, load_elem(a.vn, (int64_t)b * a.vn_sb + (int64_t)hk * a.vn_sh + tid, a.dtype), t);
    t *= inv;
    const int64_t oi = (int64_t)b * a.o_sb + (int64_t)hq * a.o_sh + tid;
    if (a.dtype == KVQ_F16) reinterpret_cast<f16*>(a.out)[oi] = (f16)t;
    else reinterpret_cast<__bf16*>(a.out)[oi] = (__bf16)t;
  }
}

// ---------------------------------------------------------------------------- merge, one round trip
// The merge above is a chain of dependent round trips (new-token dot -> (m, l) -> (m, l) again -> rows in two
// batches -> new-token V): at batch 1 nothing hides them and a call costs 5 us for 2 MB (9 us inside a decode
// step, where every operand was written by the kernel before and is cold in this XCD's L2). This variant, for up
// to kAttnBlock splits, REQUESTS everything the workgroup reads before it waits for anything — the device-side
// token count, its (m, l) pair, the new token's q / k / v elements and the first kMergePF partial rows of each
// thread (rows past the live splits are read too: the workspace holds them, their values are never used) — and
// synchronises its waves with LDS-only barriers (`__syncthreads()` would drain the outstanding global loads).
// Same arithmetic in the same order as decode_attn_merge_k: bit-identical results.
constexpr int kMergePF = 16;
// A word another kernel wrote, read through the CONSTANT address space: with a uniform address that is an s_load the
// compiler tracks itself (issued where it stands, waited for at the first use), where a global-space load becomes a
// vector load that is waited for on the spot. Only for memory no store of THIS kernel touches.
__device__ __forceinline__ int scalar_load_i32(const int* p) {
  return *reinterpret_cast<const __attribute__((address_space(4))) int*>(reinterpret_cast<uintptr_t>(p));
}
__device__ __forceinline__ void lds_barrier() {  // this workgroup's LDS traffic only; global loads stay in flight
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
// The new token's K (w = 0) / V (w = 1) slice quantised into slot T of its store by ONE workgroup, as
// quant_new_token_block does, but in one round trip: every element pair is requested up front (with the device-side
// slot number), stays in registers between the abs-max and the stores, and the workgroup meets at ONE LDS-only
// barrier. Same expressions per element (IEEE divide, round-half-even), so the stored bytes and scale are the
// generic routine's. Uniform precondition (checked by the caller): even D, 2-element-aligned rows, at most
// 2 * kAttnBlock * kNewPairs elements.
constexpr int kNewPairs = 16;
__device__ inline bool new_token_fits_registers(const NewTokenArgs& a, uint32_t w) {
  return (a.D & 1u) == 0u && (uint64_t)a.B * a.H * a.D <= 2ull * kAttnBlock * kNewPairs && ((a.xs_b[w] | a.xs_h[w]) & 1) == 0 &&
         (reinterpret_cast<uintptr_t>(a.x[w]) & 3u) == 0u;
}
template <int IDT>
__device__ inline void quant_new_token_regs(const NewTokenArgs& a, const uint32_t w, float* s_red, const int* t_dev, const uint32_t t_bound,
                                            const void* valid) {
  const uint32_t tid = threadIdx.x;
  const uint32_t np = a.B * a.H * a.D / 2u;  // element pairs
  // the device-side slot number: a SCALAR load (uniform address), issued here and waited for by the compiler at
  // its first use below the fence
  const uint32_t t_raw = (uint32_t)scalar_load_i32(t_dev ? t_dev : reinterpret_cast<const int*>(valid));
  const uint16_t* x = reinterpret_cast<const uint16_t*>(a.x[w]);
  uint32_t raw[kNewPairs];
  uint32_t row[kNewPairs], col[kNewPairs];  // (b, h) row and element offset of the pair
#pragma unroll
  for (int k = 0; k < kNewPairs; ++k) {
    const uint32_t p = tid + (uint32_t)k * kAttnBlock;
    const uint32_t e = 2u * (p < np ? p : np - 1u);
    row[k] = e / a.D;
    col[k] = e - row[k] * a.D;
    const int64_t off = (int64_t)(row[k] / a.H) * a.xs_b[w] + (int64_t)(row[k] % a.H) * a.xs_h[w] + col[k];
    raw[k] = *reinterpret_cast<const uint32_t*>(x + off);
  }
  __builtin_amdgcn_sched_barrier(0);
  const int64_t slot = t_dev ? (int64_t)(t_raw < t_bound ? t_raw : t_bound) : 0;  // host-side T: a.q / a.scale point at the slot already
  float lo[kNewPairs], hi[kNewPairs];
  float m = 0.0f;
#pragma unroll
  for (int k = 0; k < kNewPairs; ++k) {
    lo[k] = Elem<IDT>::widen((uint16_t)(raw[k] & 0xFFFFu));
    hi[k] = Elem<IDT>::widen((uint16_t)(raw[k] >> 16));
    if (tid + (uint32_t)k * kAttnBlock < np) m = fmaxf(m, fmaxf(fabsf(lo[k]), fabsf(hi[k])));
  }
  m = wave_fmax(m);
  if ((tid & 63u) == 0u) s_red[tid >> 6] = m;
  lds_barrier();
  m = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
  uint8_t* qbase = a.q[w] + slot * a.qs_t[w];
  if (a.bits[w] == 8) {
    const float s32 = fmaxf(m / QRange<8>::qmax, a.eps);
    if (tid == 0u) a.scale[w][slot] = Elem<IDT>::round_trip(s32);
#pragma unroll
    for (int k = 0; k < kNewPairs; ++k) {
      if (tid + (uint32_t)k * kAttnBlock < np) {
        uint8_t* dst = qbase + (int64_t)(row[k] / a.H) * a.qs_b[w] + (int64_t)(row[k] % a.H) * a.qs_h[w] + col[k];
        dst[0] = (uint8_t)(int8_t)quant1<8>(lo[k], s32);
        dst[1] = (uint8_t)(int8_t)quant1<8>(hi[k], s32);
      }
    }
  } else {
    const float s32 = fmaxf(m / QRange<4>::qmax, a.eps);
    if (tid == 0u) a.scale[w][slot] = Elem<IDT>::round_trip(s32);
#pragma unroll
    for (int k = 0; k < kNewPairs; ++k) {
      if (tid + (uint32_t)k * kAttnBlock < np) {
        const int h4 = quant1<4>(lo[k], s32) + 8, l4 = quant1<4>(hi[k], s32) + 8;  // even index -> high nibble
        qbase[(int64_t)(row[k] / a.H) * a.qs_b[w] + (int64_t)(row[k] % a.H) * a.qs_h[w] + (col[k] >> 1)] = (uint8_t)(((h4 & 0xF) << 4) | (l4 & 0xF));
      }
    }
  }
}

// ONE WAVE per query head (head_dim 128, at most 16 splits: what the LDS-staged kernel leaves): the same merge without the
// workgroup — lane s holds split s's (m, l), lane l holds d = l and d = 64 + l of every split's partial (32 loads, all
// requested before anything waits); the weights travel by v_readlane instead of an LDS table, and there is no barrier.
// The arithmetic, operand by operand and in the same order, is decode_attn_merge_fast_k's (its thread (g, d4) sums splits
// g, g + 8, the final row sums the 8 groups in order; its dot product sums d < 64 in wave 0 and d >= 64 in wave 1): equal bits.
// D = 64 (round 4: what the head_dim-64 ring kernel leaves): one element per lane, the block kernel's 16 split groups hold one
// split each (its dot product lives in wave 0 alone): the same chain with NH = 1.
template <uint32_t D, bool RDEV = false>
__device__ __forceinline__ void merge_one_wave(const AttnArgs& a, const bool has_new, const uint32_t hq, const uint32_t b) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  static_assert(D == 128 || D == 64, "head_dim of the one-wave merge");
  constexpr uint32_t G = 1024 / D, NSU = 16, NH = D / 64;  // the block kernel's split groups, splits held in registers, 64-element halves per lane
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t hk = hq / a.nq;
  const uint32_t nb = a.nsplit;  // 1 ... 16 (host)
  const float* ml = a.ws + ((int64_t)b * a.Hq + hq) * nb * 2;
  const float* src = a.ws + a.acc_off + ((int64_t)b * a.Hq + hq) * nb * D + lane;
  const uint32_t t_raw = (uint32_t)scalar_load_i32(a.t_dev ? a.t_dev : reinterpret_cast<const int*>(a.ws));
  const f32x2 ml_raw = __builtin_nontemporal_load(reinterpret_cast<const f32x2*>(ml) + (lane < nb ? lane : nb - 1u));
  uint16_t qraw[NH], kraw[NH], vraw[NH];
#pragma unroll
  for (int h = 0; h < (int)NH; ++h) {
    const uint32_t di = 64u * h + lane;
    qraw[h] = reinterpret_cast<const uint16_t*>(a.q)[(int64_t)b * a.q_sb + (int64_t)hq * a.q_sh + di];
    kraw[h] = reinterpret_cast<const uint16_t*>(a.kn)[(int64_t)b * a.kn_sb + (int64_t)hk * a.kn_sh + di];
    vraw[h] = reinterpret_cast<const uint16_t*>(a.vn)[(int64_t)b * a.vn_sb + (int64_t)hk * a.vn_sh + di];
  }
  float x[NH][NSU];
#pragma unroll
  for (int sp = 0; sp < (int)NSU; ++sp) {
    const uint32_t sc = (uint32_t)sp < nb ? (uint32_t)sp : nb - 1u;
#pragma unroll
    for (int h = 0; h < (int)NH; ++h) x[h][sp] = __builtin_nontemporal_load(src + (int64_t)sc * D + 64 * h);
  }
  __builtin_amdgcn_sched_barrier(0);
  const uint32_t T = a.t_dev ? (t_raw < a.T ? t_raw : a.T) : a.T;
  uint32_t ns;
  if constexpr (RDEV) {  // the ring kernel under a device-side count chose its split size from that count (its own instantiation:
    // also every device-side count with a window; the host-count instantiation never evaluates window_lo)
    const uint32_t lt = T - window_lo(a, T);  // a sliding window: the visible stored tokens (the new-token slot stays T)
    const uint32_t ns_ts = live_split_tokens(a, lt);  // evaluated in the common one, even behind a branch, it cost the batch-1 call 0.3-0.7 us)
    ns = (lt + ns_ts - 1u) / ns_ts;
  } else {
    ns = a.t_dev ? (T + a.TS - 1u) / a.TS : nb;
  }
  ns = ns < nb ? ns : nb;
  f32x2 mlv = ml_raw;
  if (lane >= ns) mlv = f32x2{-INFINITY, 0.0f};
  auto widen = [&](uint16_t h) { return a.dtype == KVQ_F16 ? Elem<KVQ_F16>::widen(h) : Elem<KVQ_BF16>::widen(h); };
  const float p0 = wave_fsum(widen(has_new ? qraw[0] : (uint16_t)0) * widen(kraw[0]));
  float p1 = 0.0f;  // the block kernel's wave 1: d >= 64 (nothing at head_dim 64)
  if constexpr (NH == 2) p1 = wave_fsum(widen(has_new ? qraw[NH - 1] : (uint16_t)0) * widen(kraw[NH - 1]));
  const float s_tok = has_new ? ((p0 + p1) + (0.0f + 0.0f)) * a.sm_scale : -INFINITY;
  const float M = fmaxf(wave_fmax(mlv[0]), s_tok);
  const float w = lane < ns ? __expf(mlv[0] - M) : 0.0f;
  const float lw = wave_fsum(lane < ns ? mlv[1] * w : 0.0f);
  const float w_new = has_new ? __expf(s_tok - M) : 0.0f;
  const float L = ((lw + 0.0f) + (0.0f + 0.0f)) + w_new;
  const float inv = 1.0f / L;
  float wt[NSU];
#pragma unroll
  for (int sp = 0; sp < (int)NSU; ++sp) wt[sp] = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(w), sp));
#pragma unroll
  for (int h = 0; h < (int)NH; ++h) {
    float t = 0.0f;
#pragma unroll
    for (int k = 0; k < (int)G; ++k) {
      float o = 0.0f;
#pragma unroll
      for (int u = 0; u < (int)(NSU / G); ++u) {
        const int sp = k + u * (int)G;
        if ((uint32_t)sp < ns) o += x[h][sp] * wt[sp];
      }
      t += o;
    }
    if (has_new) t = fmaf(w_new, widen(vraw[h]), t);
    t *= inv;
    const int64_t oi = (int64_t)b * a.o_sb + (int64_t)hq * a.o_sh + 64 * h + lane;
    if (a.dtype == KVQ_F16) reinterpret_cast<f16*>(a.out)[oi] = (f16)t;
    else reinterpret_cast<__bf16*>(a.out)[oi] = (__bf16)t;
  }
}

// (has_new: without a new token the host points kn / vn at the query, so that the three loads need no branch)
// PF: partial rows each thread requests up front (and holds): ceil(nsplit / (256 / (D/4))) rounded up to 2 / 4 / 16 by the
// host — the 16 splits per head of the LDS-staged kernel need 2, not 16 (14 clamped re-reads of the last row per thread)
template <int PF, bool RDEV = false>
__global__ __launch_bounds__(kAttnBlock) void decode_attn_merge_fast_k(const AttnArgs a, const NewTokenArgs nt, const int fuse_quant_i,
                                                                       const int has_new_i) {
  __shared__ float s_red[3][kAttnBlock / kWave];
  // fuse_quant_i bit 0: the launch's last two workgroups quantise-append the new token; bit 1 (PF == 2, head_dim 128, <= 16
  // splits): ONE WAVE per head, four heads per workgroup (merge_one_wave)
  const int fuse_quant = fuse_quant_i & 1;
  const bool by_wave = PF == 2 && (fuse_quant_i & 2) != 0;
  const uint32_t n_head_wgs = by_wave ? (a.Hq + 3u) / 4u : a.Hq;
  if (blockIdx.x >= n_head_wgs) {  // new-token workgroups: (K | V) x pieces (one piece unless nt.nparts > 1)
    const uint32_t idx_new_tok = blockIdx.x - n_head_wgs, w_new_tok = idx_new_tok & 1u;
    if (fuse_quant && blockIdx.y == 0u && nt.nparts > 1u) {
      NewTokenArgs slot = nt;
      if (a.t_dev) {
        const int64_t T = (int64_t)live_tokens(a);
#pragma unroll
        for (int w = 0; w < 2; ++w) {
          slot.q[w] += T * nt.qs_t[w];
          slot.scale[w] += T;
        }
      }
      if (a.dtype == KVQ_F16) quant_new_token_parts<KVQ_F16>(slot, w_new_tok, idx_new_tok >> 1, s_red[0]);
      else quant_new_token_parts<KVQ_BF16>(slot, w_new_tok, idx_new_tok >> 1, s_red[0]);
    } else if (fuse_quant && blockIdx.y == 0u && new_token_fits_registers(nt, w_new_tok)) {
      if (a.dtype == KVQ_F16) quant_new_token_regs<KVQ_F16>(nt, w_new_tok, s_red[0], a.t_dev, a.T, a.q);
      else quant_new_token_regs<KVQ_BF16>(nt, w_new_tok, s_red[0], a.t_dev, a.T, a.q);
    } else if (fuse_quant && blockIdx.y == 0u) {
      NewTokenArgs slot = nt;
      if (a.t_dev) {
        const int64_t T = (int64_t)live_tokens(a);
#pragma unroll
        for (int w = 0; w < 2; ++w) {
          slot.q[w] += T * nt.qs_t[w];
          slot.scale[w] += T;
        }
      }
      if (a.dtype == KVQ_F16) quant_new_token_block<KVQ_F16>(slot, w_new_tok, s_red[0]);
      else quant_new_token_block<KVQ_BF16>(slot, w_new_tok, s_red[0]);
    }
    return;
  }
  if constexpr (PF == 2) {
    if (by_wave) {
      const uint32_t hq_w = blockIdx.x * 4u + (threadIdx.x >> 6);
      if (hq_w < a.Hq) {
        if (a.D == 128u) merge_one_wave<128, RDEV>(a, has_new_i != 0, hq_w, blockIdx.y);
        else merge_one_wave<64, RDEV>(a, has_new_i != 0, hq_w, blockIdx.y);
      }
      return;
    }
  }
  __shared__ float s_wt[kAttnBlock];
  __shared__ __attribute__((aligned(16))) float s_out[kAttnBlock * 4];
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const uint32_t tid = threadIdx.x;
  const uint32_t hq = blockIdx.x, b = blockIdx.y;
  const uint32_t hk = hq / a.nq;
  const bool has_new = has_new_i != 0;
  const uint32_t wave = tid >> 6, lane = tid & 63u;
  const uint32_t nb = a.nsplit;  // 1 ... kAttnBlock (host); the row stride of the partials
  const uint32_t dv = a.D >> 2;
  const uint32_t groups = kAttnBlock / dv;  // 32, 16, 8 or 4
  const uint32_t g = tid / dv, d4 = tid - g * dv;
  const float* ml = a.ws + ((int64_t)b * a.Hq + hq) * nb * 2;
  const f32x4* src = reinterpret_cast<const f32x4*>(a.ws + a.acc_off + ((int64_t)b * a.Hq + hq) * nb * a.D) + d4;

  // ---- requests: straight-line code (clamped indices, selected addresses), nothing waits before the fence -------
  // the device-side token count: a SCALAR buffer load (uniform address; a plain `*a.t_dev` becomes a vector load that is
  // waited for on the spot), issued here and waited for by the compiler at its first use below the fence
  const uint32_t t_raw = (uint32_t)scalar_load_i32(a.t_dev ? a.t_dev : reinterpret_cast<const int*>(a.ws));
  const f32x2 ml_raw = __builtin_nontemporal_load(reinterpret_cast<const f32x2*>(ml) + (tid < nb ? tid : nb - 1u));
  const uint32_t di = tid < a.D ? tid : a.D - 1u;
  const uint16_t qb_raw = reinterpret_cast<const uint16_t*>(a.q)[(int64_t)b * a.q_sb + (int64_t)hq * a.q_sh + di];
  const uint16_t kb = reinterpret_cast<const uint16_t*>(a.kn)[(int64_t)b * a.kn_sb + (int64_t)hk * a.kn_sh + di];
  const uint16_t vb = reinterpret_cast<const uint16_t*>(a.vn)[(int64_t)b * a.vn_sb + (int64_t)hk * a.vn_sh + di];
  f32x4 x[PF];
#pragma unroll
  for (int u = 0; u < PF; ++u) {
    const uint32_t s = g + (uint32_t)u * groups;
    x[u] = __builtin_nontemporal_load(src + (int64_t)(s < nb ? s : nb - 1u) * dv);
  }
  __builtin_amdgcn_sched_barrier(0);
  const uint32_t T = a.t_dev ? (t_raw < a.T ? t_raw : a.T) : a.T;
  const uint16_t qb = (has_new && tid < a.D) ? qb_raw : (uint16_t)0;  // the dot product runs over d < D
  f32x2 mlv = ml_raw;

  // ---- weights ---------------------------------------------------------------------------------------------
  uint32_t ns;
  if constexpr (RDEV) {  // the ring kernel under a device-side count chose its split size from that count (its own instantiation:
    // also every device-side count with a window; the host-count instantiation never evaluates window_lo)
    const uint32_t lt = T - window_lo(a, T);  // a sliding window: the visible stored tokens (the new-token slot stays T)
    const uint32_t ns_ts = live_split_tokens(a, lt);  // evaluated in the common one, even behind a branch, it cost the batch-1 call 0.3-0.7 us)
    ns = (lt + ns_ts - 1u) / ns_ts;
  } else {
    ns = a.t_dev ? (T + a.TS - 1u) / a.TS : nb;
  }
  ns = ns < nb ? ns : nb;
  if (tid >= ns) mlv = f32x2{-INFINITY, 0.0f};
  auto widen = [&](uint16_t h) { return a.dtype == KVQ_F16 ? Elem<KVQ_F16>::widen(h) : Elem<KVQ_BF16>::widen(h); };
  {
    const float part = wave_fsum(widen(qb) * widen(kb));  // zero beyond D and without a new token
    const float mw = wave_fmax(mlv[0]);
    if (lane == 0u) {
      s_red[0][wave] = part;
      s_red[1][wave] = mw;
    }
  }
  lds_barrier();
  const float s_tok = has_new ? ((s_red[0][0] + s_red[0][1]) + (s_red[0][2] + s_red[0][3])) * a.sm_scale : -INFINITY;
  const float M = fmaxf(fmaxf(fmaxf(s_red[1][0], s_red[1][1]), fmaxf(s_red[1][2], s_red[1][3])), s_tok);
  {
    const float w = tid < ns ? __expf(mlv[0] - M) : 0.0f;
    s_wt[tid] = w;
    const float lw = wave_fsum(tid < ns ? mlv[1] * w : 0.0f);
    if (lane == 0u) s_red[2][wave] = lw;
  }
  lds_barrier();  // also publishes s_wt
  const float w_new = has_new ? __expf(s_tok - M) : 0.0f;
  const float L = ((s_red[2][0] + s_red[2][1]) + (s_red[2][2] + s_red[2][3])) + w_new;
  const float inv = 1.0f / L;

  // ---- weighted sum: thread = (split group g, 4 elements at d4) ---------------------------------------------
  f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int u = 0; u < PF; ++u) {
    const uint32_t s = g + (uint32_t)u * groups;
    if (s < ns) o += x[u] * s_wt[s];
  }
  for (uint32_t s = g + (uint32_t)PF * groups; s < ns; s += groups) o += src[(int64_t)s * dv] * s_wt[s];
  *reinterpret_cast<f32x4*>(&s_out[tid * 4]) = o;  // [g][d]
  lds_barrier();
  if (tid < a.D) {
    float t = 0.0f;
    for (uint32_t k = 0; k < groups; ++k) t += s_out[k * a.D + tid];
    if (has_new) t = fmaf(w_new, widen(vb), t);
    t *= inv;
    const int64_t oi = (int64_t)b * a.o_sb + (int64_t)hq * a.o_sh + tid;
    if (a.dtype == KVQ_F16) reinterpret_cast<f16*>(a.out)[oi] = (f16)t;
    else reinterpret_cast<__bf16*>(a.out)[oi] = (__bf16)t;
  }
}

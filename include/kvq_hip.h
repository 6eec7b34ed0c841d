/*
 * kvq_hip.h — C ABI of libkvq_hip.so: MI355X (gfx950) KV-cache quantize / dequantize /
 * eviction kernels.
 *
 * This is the drop-in boundary for the reference's native plugin `kvq_ext`
 * (reference src/cuda/extensions.py:116-119, a pybind11 module JIT-built from an inline
 * CUDA string) and for the torch-op arithmetic of src/quantization/ops.py and
 * src/cache/implementations.py that the MI355X build moves into HIP.
 *
 * Conventions
 *   - plain C: raw device pointers, sizes, strides; no torch / C++ types.
 *   - the library never allocates, frees or retains memory; every buffer is the caller's.
 *   - every entry point returns 0 on success, a negative KVQ_E_* code for argument errors,
 *     or a positive hipError_t for launch errors; kvq_last_error_string() describes the last
 *     failure on the calling thread.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream). All work is
 *     enqueued asynchronously; there is NO host synchronisation anywhere on the path
 *     (the reference syncs once per call through float(scale), ops.py:87,117).
 *   - stateless and re-entrant; safe to call from several host threads.
 *
 * KV views.  A KV tensor set is addressed as [G, B, H, T, D] with the last dim contiguous:
 *   G  independent scale groups (layer x K|V); never share a scale
 *   B,H batch rows and heads; ONE scale spans all B*H*D values of a token (ops.py:27,48:
 *       abs().max() over the whole [B,H,1,D] slice)
 *   T  tokens, D head_dim.
 * Strides are in ELEMENTS of the pointed-to type. The reference's legacy tuple
 * tuple_L[(k, v)] of [B,H,T,D] tensors (ops.py:178-179,217) is G = 2L views that live in
 * separate allocations: pass them as a host array of G device pointers (`*_ptrs`), or pass a
 * single base + strides.g when they are one buffer.
 *
 * Scale tables.  scales[g * scale_stride_g + t] is the STORED scale of token t widened to
 * fp32: the reference computes the scale in fp32, quantises with that fp32 value and stores
 * it rounded to the input dtype (ops.py:26-30,47-50,65); dequantisation widens the stored
 * value (ops.py:87,90,117,133). The quantise kernels reproduce exactly that split.
 */
#ifndef KVQ_HIP_H
#define KVQ_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KVQ_VERSION 100 /* 0.1.0 */

/* floating-point element types of KV tensors */
#define KVQ_F16 0
#define KVQ_BF16 1
#define KVQ_F32 2

/* argument errors (negative); launch errors are positive hipError_t values */
#define KVQ_E_NULL (-1)      /* required pointer is NULL */
#define KVQ_E_DIMS (-2)      /* negative / inconsistent dims or strides */
#define KVQ_E_DTYPE (-3)     /* unknown dtype code */
#define KVQ_E_DEVICE (-4)    /* the output buffer lives on another device than the calling thread's current one */

/* Pointer-list entry points take any number of groups; they launch once per 128 pointers
 * (the pointers travel by value in the kernel-argument segment). */

typedef struct {
  int64_t G, B, H, T, D;
} kvq_dims_t;

typedef struct {
  int64_t g, b, h, t; /* element strides; the D stride is 1 */
} kvq_strides_t;

int kvq_version(void);
const char* kvq_last_error_string(void);

/* ---- reference-equivalent flat entry points (one host scalar scale per launch) ---------- */

/* Replaces kvq_ext.dequant_int8_to_fp16(Tensor q, double scale) — extensions.py:70-86,
 * kernel :37-48: out[i] = half(float(q[i]) * scale), n elements, q and out contiguous. */
int kvq_dequant_i8_f16_flat(const int8_t* q, float scale, void* out_f16, int64_t n, void* stream);

/* Replaces kvq_ext.dequant_int4_packed_to_fp16(Tensor packed, double scale, int64 orig_last_dim)
 * — extensions.py:88-114, kernel :50-68. `packed` holds n_packed bytes, rows of `packed_last`
 * bytes; out holds 2*n_packed halves, rows of 2*packed_last. Even index = HIGH nibble (:61),
 * value (nibble-8)*scale, columns >= orig_last_dim written as 0 (:65-66). */
int kvq_dequant_i4_f16_flat(const uint8_t* packed, float scale, void* out_f16, int64_t n_packed,
                            int64_t packed_last, int64_t orig_last_dim, void* stream);

/* ---- token-table dequantise: a whole layer set per launch -------------------------------- */

/* Replaces the 2*L*T per-slice dequantize_int8_per_tensor calls + T-way torch.cat of
 * QuantizedLayerKV.get_kv (ops.py:213-269) / QuantizedKVCache.to_past_key_values (:345-355).
 * q [G,B,H,T,D] int8 (strides q_st) -> out [G,B,H,T,D] of out_dtype (strides out_st).
 * out = RN_out(float(q) * scales[g,t]). */
int kvq_dequant_i8_tokens(const int8_t* q, const kvq_strides_t* q_st, const float* scales,
                          int64_t scale_stride_g, void* out, const kvq_strides_t* out_st,
                          int out_dtype, const kvq_dims_t* dims, void* stream);

/* Same for packed INT4 (dequantize_int4_per_tensor_packed, ops.py:93-133). dims->D is the
 * UNPACKED head_dim (orig_last_dim); packed rows hold (D+1)/2 bytes; p_st strides are in bytes. */
int kvq_dequant_i4_tokens(const uint8_t* packed, const kvq_strides_t* p_st, const float* scales,
                          int64_t scale_stride_g, void* out, const kvq_strides_t* out_st,
                          int out_dtype, const kvq_dims_t* dims, void* stream);

/* ---- token-table quantise ---------------------------------------------------------------- */

/* NON-FINITE INPUT — one rule for every quantise route, the reference's own (torch's abs().max() and clamp(min=eps) keep
 * a NaN; its cast of a NaN quotient to int8 stores 0). No entry point has a "finite inputs" precondition:
 *   - A token slice [B,H,1,D] that holds a NaN or an inf stores code 0 in EVERY element (INT8 0x00, packed INT4 0x88, the
 *     pad nibble of an odd D included) and the scale NaN if the slice holds a NaN, else +inf. The token dequantises to NaN
 *     throughout (0 * inf, anything * NaN): loud, and contained to that token — the other tokens of the tensor keep their
 *     ordinary bits, whatever tile, wave or workgroup they share with it.
 *   - Abs-max tables (kvq_absmax_tokens): NaN for a slice with a NaN, else +inf for one with an inf. kvq_absmax_tokens_acc
 *     also keeps a NaN the table already holds.
 *   - Caller-given tables (kvq_quant_tokens_from_absmax): under a finite entry +inf / -inf clamp to QMAX / QMIN like any
 *     quotient past the range and a NaN element is code 0; a NaN or +inf entry gives code 0 throughout and that scale.
 *   - The decode step's new token (kvq_decode_step*, every routine and batch size) and the summary token of
 *     kvq_store_chunk_pool (a chunk with a NaN- or inf-scale token pools to a NaN mean: code 0, scale NaN) follow the
 *     first rule; kept tail tokens move with their raw bits.
 * Which NaN (sign, payload) a scale or table word holds is not specified. */

/* Replaces quantize_int8_per_tensor (ops.py:10-30) applied per token slice by
 * QuantizedLayerKV.append (ops.py:174-210) under init_from_prompt_past (:333-342) /
 * append_from_past (:323-330).
 *   in:  [G,B,H,T,D] of in_dtype. Either in_ptrs (HOST array of G device pointers, strides.g
 *        ignored) or in_base (+ in_st->g); exactly one of them non-NULL.
 *   q:   [G,B,H,T,D] int8 store, strides q_st (a window of a larger [.., Tcap, D] store).
 *   scales: stored scale widened to fp32, scales[g*scale_stride_g + t].
 *   absmax_ws: caller workspace of G*T floats (used by the two-pass path; contents undefined
 *        afterwards).
 *   s32 = max(max|x| / 127, eps) in fp32; q = clamp(rint(x / s32), -127, 127);
 *   stored = RN_in_dtype(s32). NaN / inf in x: the rule above (code 0, scale NaN / +inf for that token). */
int kvq_quant_i8_tokens(const void* in_base, const void* const* in_ptrs, const kvq_strides_t* in_st,
                        int in_dtype, int8_t* q, const kvq_strides_t* q_st, float* scales,
                        int64_t scale_stride_g, float* absmax_ws, float eps,
                        const kvq_dims_t* dims, void* stream);

/* Same for quantize_int4_per_tensor_packed (ops.py:33-65): s32 = max(max|x|/7, eps);
 * q = clamp(rint(x/s32), -8, 7); nibble = q+8; even d -> high nibble; odd D padded with
 * nibble 8 (ops.py:54-59). packed rows hold (D+1)/2 bytes; p_st in bytes. NaN / inf in x: every byte of the token 0x88. */
int kvq_quant_i4_tokens(const void* in_base, const void* const* in_ptrs, const kvq_strides_t* in_st,
                        int in_dtype, uint8_t* packed, const kvq_strides_t* p_st, float* scales,
                        int64_t scale_stride_g, float* absmax_ws, float eps,
                        const kvq_dims_t* dims, void* stream);

/* ---- split phases: a batched slice whose batch rows are sharded over ranks -------------------- */

/* The reference's scale spans the WHOLE [B,H,1,D] slice (ops.py:27,48), so when B is split over ranks
 *  the abs-max must cross ranks between the reduction and the quantisation:
 *   kvq_absmax_tokens            local rows -> absmax[g*T + t] = max |x| over this rank's [B_local,H,D]
 *   all_reduce(MAX) of absmax    (the caller's collective: RCCL over xGMI, torch.distributed)
 *   kvq_quant_tokens_from_absmax quantise the local rows with scale max(absmax/QMAX, eps), store the scale
 * On one rank (no all_reduce) the pair is bit-identical with kvq_quant_i8_tokens / kvq_quant_i4_tokens.
 * absmax: contiguous [G,T] fp32, overwritten by phase 1 (no pre-initialisation needed). An entry is NaN when the slice holds
 * a NaN, else +inf when it holds an inf (the rule above). What a collective's MAX does with a NaN is the collective's. */
int kvq_absmax_tokens(const void* in_base, const void* const* in_ptrs, const kvq_strides_t* in_st, int in_dtype,
                      float* absmax, const kvq_dims_t* dims, void* stream);

/* kvq_absmax_tokens without the fill: absmax[g*T + t] = max(absmax[g*T + t], max |x| over this rank's [B_local,H,D]).
 * The caller initialises the table (non-negative values; zeros for a plain abs-max): a layer-chunked pass zeroes its
 * whole [G,T] table with ONE fill instead of one per chunk (a fill is a launch: 4.5 us each on MI355X). A NaN on either
 * side — in the data or already in the table — stays; +inf is a value. */
int kvq_absmax_tokens_acc(const void* in_base, const void* const* in_ptrs, const kvq_strides_t* in_st, int in_dtype,
                          float* absmax, const kvq_dims_t* dims, void* stream);

/* bits: 8 (int8 store, strides in bytes = elements) or 4 (packed store, (D+1)/2 bytes per row).
 * absmax may be any non-negative table, also one SMALLER than the data (a static or calibrated scale table): every route
 * clamps q to [QMIN, QMAX] like the reference, so all of them store the same bytes. Only these routes need the clamp: a
 * kernel that takes the abs-max of the data itself bounds |x / s32| by QMAX (1 + 2^-23), which rounds to QMAX.
 * Non-finite (the rule above): a finite entry clamps +inf / -inf to QMAX / QMIN and stores a NaN element as 0; a NaN or +inf
 * entry stores code 0 throughout and that scale. */
int kvq_quant_tokens_from_absmax(int bits, const void* in_base, const void* const* in_ptrs, const kvq_strides_t* in_st,
                                 int in_dtype, uint8_t* q, const kvq_strides_t* q_st, float* scales,
                                 int64_t scale_stride_g, const float* absmax, float eps, const kvq_dims_t* dims,
                                 void* stream);

/* ---- eviction ---------------------------------------------------------------------------- */

/* Replaces trim_kv_sliding_window (src/cache/implementations.py:124-140), materialised:
 * out[g,b,h,0:W,:] = in[g,b,h,T-W:T,:] with W = min(window, T). The reference returns views
 * and leaves the byte movement to the next torch.cat; a persistent buffer must compact.
 * in and out must not overlap. elem_size is 2 or 4 bytes. A pointer list goes 128 groups per launch; a single base with
 * in_st->g (one allocation: e.g. a paged pool's blocks) is ONE launch for up to 65,535 groups. */
int kvq_window_compact(const void* in_base, const void* const* in_ptrs, const kvq_strides_t* in_st,
                       void* out, const kvq_strides_t* out_st, int elem_size, int64_t window,
                       const kvq_dims_t* dims, void* stream);

/* Replaces chunk_summarize_kv (implementations.py:295-346) on [G,B,H,T,D]:
 *   keep = min(keep_last, T); old = T - keep; n = ceil(old / chunk_size)
 *   out[.., j, :]     = RN_dtype( (sum_{i<chunk_size, j*chunk_size+i<old} in[.., j*chunk_size+i, :]) / chunk_size )   j < n
 *   out[.., n + i, :] = in[.., old + i, :]                                                  i < keep
 * fp32 accumulation, sequential in t; divisor is chunk_size even for the ragged last chunk
 * (zero padding, :326-333). If old <= 0 the call copies in to out unchanged (T rows).
 * Output has kvq_chunk_summary_len(T, chunk_size, keep_last) tokens. */
int kvq_chunk_meanpool(const void* in_base, const void* const* in_ptrs, const kvq_strides_t* in_st,
                       void* out, const kvq_strides_t* out_st, int dtype, int64_t chunk_size,
                       int64_t keep_last, const kvq_dims_t* dims, void* stream);

int64_t kvq_chunk_summary_len(int64_t T, int64_t chunk_size, int64_t keep_last);

/* Replaces the index_select + torch.cat of the sparse eviction family — trim_kv_prefix_window,
 * trim_kv_strided, trim_kv_block_old, trim_kv_budget_old (src/cache/implementations.py:143-292):
 *   out[g,b,h,j,:] = in[g,b,h,idx[j],:]   j < n_idx
 * idx is a DEVICE array of n_idx int32 token indices in [0, dims->T) (built by the host from the
 * policy). The kernel compares every index with dims->T: an index outside the range yields a row of
 * zeros, never an out-of-bounds read (torch's index_select raises there; the Python wrappers validate
 * host-built index lists before the call). elem_size is 2 or 4 bytes. */
int kvq_gather_tokens(const void* in_base, const void* const* in_ptrs, const kvq_strides_t* in_st,
                      void* out, const kvq_strides_t* out_st, int elem_size, const int32_t* idx,
                      int64_t n_idx, const kvq_dims_t* dims, void* stream);

/* chunk_summarize_kv applied to a QUANTISED store, inside the quantised domain: no fp16 copy of the store exists.
 *   q_in  [G,B,H,T,Dq] codes (int8, or packed INT4: Dq = (D+1)/2, even element in the high nibble), BYTE strides q_in_st;
 *   scales_in[g * scale_in_stride_g + t] the stored scales; q_out [G,B,H,Tout,Dq] / scales_out likewise,
 *   Tout = kvq_chunk_summary_len(T, chunk_size, keep_last). dims->D is the UNPACKED head_dim. dtype (KVQ_F16 | KVQ_BF16)
 *   is the dtype the store was quantised from (the one its scales are rounded to).
 * The result is the composition kvq_dequant_*_tokens -> kvq_chunk_meanpool -> kvq_quant_*_tokens, bit for bit. With
 * keep = min(keep_last, T), old = T - keep, n = ceil(old / chunk_size):
 *   pooled row j < n:  x[t] = RN_dtype(float(code[t]) * scales_in[g,t])
 *                      m    = RN_dtype((fp32 sum of x[t] over the chunk, sequential in t from +0.0) / (float)chunk_size)
 *                             (the divisor is chunk_size for the ragged last chunk too; an IEEE divide)
 *                      s32  = max(max |m| over ALL b, h, d of the group / QMAX, eps)
 *                      code' = clamp(rint(m / s32), QMIN, QMAX); scales_out[g,j] = float(RN_dtype(s32))
 *                      INT4 nibble order and the pad nibble 8 of an odd D as kvq_quant_i4_tokens writes them
 *   tail row j >= n:   the RAW code bytes and the RAW scale word of token old + (j - n): kept tokens are not requantised
 *   old <= 0:          a copy of all T rows.
 * A chunk token whose scale is NaN or +inf (a poisoned token, as the quantise calls store it) makes the mean NaN: the pooled
 * token is code 0 under a NaN scale, as the composition gives it; tail tokens keep their raw NaN / inf scale words.
 * Out of place: overlapping input and output ranges (codes or scales) return KVQ_E_DIMS. One workgroup owns one pooled
 * token of one group (the whole [B,H,D] slice), so the abs-max never leaves it: one launch, no workspace. A slice of
 * more than 8,192 elements (B * H * D) returns KVQ_E_DIMS and the error string says so: compose the three calls above.
 * Kernels: store_pool_fast_k (D % 32 == 0, 16-byte aligned rows and strides: 16-byte non-temporal loads, a batch of
 * chunk rows in flight per lane, pooled values in registers, 16-byte stores; 8-byte pieces for an INT4 slice of at most 32
 * 16-byte pieces, so that a whole wave works) or store_pool_generic_k (any other layout;
 * pooled values in LDS). Also refused before any launch: NULL pointers, negative or >= 2^31 dims, bits other than 4 / 8,
 * dtype other than fp16 / bf16 (KVQ_E_DTYPE), chunk_size <= 0, keep_last < 0, outputs on another device. */
int kvq_store_chunk_pool(int bits, const uint8_t* q_in, const kvq_strides_t* q_in_st, const float* scales_in,
                         int64_t scale_in_stride_g, uint8_t* q_out, const kvq_strides_t* q_out_st, float* scales_out,
                         int64_t scale_out_stride_g, int dtype, int64_t chunk_size, int64_t keep_last, float eps,
                         const kvq_dims_t* dims, void* stream);

/* ---- decode attention over the quantised store -------------------------- */

typedef struct {
  int64_t B, Hq, Hkv, T, D; /* T = stored (quantised) tokens attended; Hq % Hkv == 0, Hq/Hkv <= 8 (<= 16 at head_dim 64 / 128) */
} kvq_attn_dims_t;

/* Workspace floats kvq_decode_attn needs for these dims (-1 on bad dims). */
int64_t kvq_decode_attn_workspace(const kvq_attn_dims_t* dims);
/* Largest kvq_decode_attn_workspace over every T' <= dims->T (it is not monotone in T): what a decode
 * loop allocates once for its reserved capacity. */
int64_t kvq_decode_attn_workspace_cap(const kvq_attn_dims_t* dims);

/* One decode step of one layer without materialising the fp16 cache. Replaces, for a single
 * query token, QuantizedKVCache.to_past_key_values (src/quantization/ops.py:345-355: dequantise
 * every stored token) + the model's attention over [dequantised past, new token]
 * (src/benchmarking/benchmarker.py:470-471):
 *   s[t]   = sm_scale * k_scales[t] * sum_d q[d] * k_int[t,d]            t < T
 *   s_new  = sm_scale * sum_d q[d] * k_new[d]                             (if k_new)
 *   p      = softmax over {s[0..T), s_new}
 *   out[d] = sum_t p[t] * v_scales[t] * v_int[t,d] + p_new * v_new[d]
 * q / k_new / v_new / out: [B, H, D] of `dtype` (KVQ_F16 | KVQ_BF16) with element strides
 * (stride_b, stride_h), D contiguous; q heads Hq, k_new / v_new heads Hkv; query head h uses kv
 * head h / (Hq/Hkv). k_store / v_store: one layer's [B, Hkv, Tcap, Dq] rows (int8, or packed INT4
 * with the even element in the high nibble), byte strides k_st / v_st (g unused); *_scales[t] the
 * per-token scale table of that layer. k_bits / v_bits: 8 or 4. D in {32, 64, 128, 256}.
 * fp32 accumulation; the reference's intermediate fp16 rounding of the dequantised values is
 * skipped, so results agree within fp16 tolerance, not bit-exactly. */
int kvq_decode_attn(const void* q, int64_t q_stride_b, int64_t q_stride_h,
                    const uint8_t* k_store, const kvq_strides_t* k_st, const float* k_scales, int k_bits,
                    const uint8_t* v_store, const kvq_strides_t* v_st, const float* v_scales, int v_bits,
                    const void* k_new, int64_t kn_stride_b, int64_t kn_stride_h,
                    const void* v_new, int64_t vn_stride_b, int64_t vn_stride_h,
                    void* out, int64_t out_stride_b, int64_t out_stride_h, int dtype, float sm_scale,
                    float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* dims, void* stream);

/* kvq_decode_attn over the T stored tokens + the new token, THEN the new token's K / V quantised into
 * slot T of the stores (scales[T]): everything one layer does per decode step in the reference
 * (append_from_past ops.py:323-330, to_past_key_values :345-355, attention) behind one call.
 * The caller guarantees capacity for slot T (k_st / v_st describe the whole [B,Hkv,Tcap,Dq] store)
 * and counts the token as stored afterwards. workspace as for kvq_decode_attn (>= 1 float).
 * Two launches: the new token is quantised by two extra workgroups of the merge launch.
 * The workspace needs no initialisation. A NaN or inf in k_new / v_new: slot T stores code 0 and the scale NaN / +inf (the
 * quantise rule above), whichever routine the slice size picks; the attention output of that step is then not finite. */
int kvq_decode_step(const void* q, int64_t q_stride_b, int64_t q_stride_h,
                    const void* k_new, int64_t kn_stride_b, int64_t kn_stride_h,
                    const void* v_new, int64_t vn_stride_b, int64_t vn_stride_h,
                    uint8_t* k_store, const kvq_strides_t* k_st, float* k_scales, int k_bits,
                    uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales, int v_bits,
                    void* out, int64_t out_stride_b, int64_t out_stride_h, int dtype, float sm_scale, float eps,
                    float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* dims, void* stream);

/* kvq_decode_step with the stored-token count in DEVICE memory: every argument of the two launches is then the
 * same from one decode step to the next, so a HIP graph that captured the step (together with the model's own
 * kernels) can be replayed for every later token — the host loop of the reference's generate_with_quantized_kv
 * (src/benchmarking/benchmarker.py:465-486) leaves the critical path. `*t_dev` (int32) = tokens stored before
 * the step; the caller increments it on the same stream afterwards. dims->T is the HOST's upper bound on
 * *t_dev (e.g. the store's capacity - 1): it sizes the grid and the workspace (kvq_decode_attn_workspace for
 * that T); workgroups beyond the live count exit at once. The caller guarantees *t_dev <= dims->T and room for
 * slot *t_dev. One-tile kernels only (no streaming / fused variants); B * Hkv * D <= 65536. */
int kvq_decode_step_dev(const void* q, int64_t q_stride_b, int64_t q_stride_h,
                        const void* k_new, int64_t kn_stride_b, int64_t kn_stride_h,
                        const void* v_new, int64_t vn_stride_b, int64_t vn_stride_h,
                        uint8_t* k_store, const kvq_strides_t* k_st, float* k_scales, int k_bits,
                        uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales, int v_bits,
                        void* out, int64_t out_stride_b, int64_t out_stride_h, int dtype, float sm_scale, float eps,
                        float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* dims, const int32_t* t_dev,
                        void* stream);

/* kvq_decode_step (append != 0) or kvq_decode_attn with the new token given (append == 0) for n_layers
 * layers behind ONE host call: the per-layer launches are enqueued back to back on `stream`, so a decode step costs one trip through the binding instead of one per
 * layer — the reference pays 2*T Python-level calls per layer and step here (ops.py:345-355). Every
 * pointer argument is a HOST array of n_layers device pointers; dims, strides, kinds and dtype are
 * shared by all layers; `workspace` is reused by consecutive launches (stream order makes that safe).
 * k_new / v_new may be NULL when append == 0 (attention over the stored tokens only). */
int kvq_decode_step_layers(int64_t n_layers, int append, const void* const* q, int64_t q_stride_b, int64_t q_stride_h,
                           const void* const* k_new, int64_t kn_stride_b, int64_t kn_stride_h,
                           const void* const* v_new, int64_t vn_stride_b, int64_t vn_stride_h,
                           uint8_t* const* k_store, const kvq_strides_t* k_st, float* const* k_scales, int k_bits,
                           uint8_t* const* v_store, const kvq_strides_t* v_st, float* const* v_scales, int v_bits,
                           void* const* out, int64_t out_stride_b, int64_t out_stride_h, int dtype, float sm_scale,
                           float eps, float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* dims,
                           void* stream);

/* ---- multi-token causal attention over the quantised store (chunked prefill, speculative verify) ---- */

typedef struct {
  int64_t B, Hq, Hkv, T, S, D; /* T = stored tokens attended (>= 0), S = new query tokens (>= 1); Hq % Hkv == 0,
                                  Hq/Hkv <= 16; D in {64, 128} */
} kvq_extend_dims_t;

/* Workspace floats kvq_extend_attn needs for these dims (-1 on bad dims; 0 = none). Non-decreasing in T for fixed
 * B, Hq, Hkv, S, D: a size taken at the store's capacity covers every shorter context. */
int64_t kvq_extend_attn_workspace(const kvq_extend_dims_t* dims);

/* S new tokens of one layer attend the T stored tokens and, causally, themselves — what the reference computes for a
 * multi-token forward over a dequantised past (src/quantization/ops.py:345-355 + the model's attention with HF's
 * lower-right-aligned causal mask), without materialising the fp16 cache. For query row s (0 <= s < S):
 *   s_st[t]  = sm_scale * k_scales[t] * sum_d q[s,d] * k_int[t,d]            t < T
 *   s_new[j] = sm_scale * sum_d q[s,d] * k_new[j,d]                            j <= s
 *   out[s]   = softmax over {s_st, s_new} applied to v_scales[t] * v_int[t] / v_new[j]
 * q / out: [B, Hq, S, D] and k_new / v_new: [B, Hkv, S, D] of `dtype` (KVQ_F16 | KVQ_BF16) with element strides
 * (b, h, s), D contiguous, 16-byte aligned, every stride a multiple of 8 elements (HF's [B, S, H, D] projections and
 * output pass without a copy); query head h uses kv head h / (Hq/Hkv). k_store / v_store / scales as for kvq_decode_attn
 * (tokens [0, T) are read, nothing past them). The chunk is NOT appended to the store: quantise it with
 * kvq_quant_*_tokens into slots T .. T+S-1 (bit-identical to a whole-prompt quantise). fp32 accumulation; P rounded
 * to `dtype` for the matrix cores, so results agree with the reference within fp16 / bf16 tolerance. One launch, plus a
 * merge launch when the stored tokens are split. The workspace needs no initialisation. */
int kvq_extend_attn(const void* q, int64_t q_stride_b, int64_t q_stride_h, int64_t q_stride_s,
                    const uint8_t* k_store, const kvq_strides_t* k_st, const float* k_scales, int k_bits,
                    const uint8_t* v_store, const kvq_strides_t* v_st, const float* v_scales, int v_bits,
                    const void* k_new, int64_t kn_stride_b, int64_t kn_stride_h, int64_t kn_stride_s,
                    const void* v_new, int64_t vn_stride_b, int64_t vn_stride_h, int64_t vn_stride_s,
                    void* out, int64_t out_stride_b, int64_t out_stride_h, int64_t out_stride_s, int dtype,
                    float sm_scale, float* workspace, int64_t workspace_floats, const kvq_extend_dims_t* dims,
                    void* stream);

/* Sliding-window attention over the store (HF's sliding_window: a query at absolute position p sees key k iff
 * p - W < k <= p, W keys with its own). Each entry point takes the arguments of its unwindowed counterpart plus
 * `window` (W) directly after sm_scale. window = 0: no window, exactly the unwindowed call; window < 0: KVQ_E_DIMS.
 * The store keeps every token; a window only limits what is read:
 *   kvq_decode_attn_window      query at position T with k_new (stored [lo, T) + the new token, lo = max(0, T + 1 - W)),
 *                               at T - 1 without (the last stored token is its own; lo = max(0, T - W)).
 *   kvq_decode_step_window      as kvq_decode_attn_window with the new token; the new token is still quantised into
 *                               slot T, bit-identical to kvq_decode_step.
 *   kvq_decode_step_dev_window  lo derived on the device from *t_dev with the same formula; the grid is planned for
 *                               min(dims->T, W - 1) stored tokens, the count and the new-token slot are still clamped to
 *                               dims->T. A live count of 0 (W = 1, or *t_dev = 0) gives the new token's V.
 *   kvq_extend_attn_window      query row s at position T + s sees stored t >= T + s + 1 - W and chunk tokens
 *                               s - W < j <= s (the chunk itself is banded when S > W).
 * CONTRACT: stored tokens before lo (decode) or before max(0, T + 1 - W) (extend) are never read, neither codes nor
 * scales; they may hold anything.
 * Host-count decode with a window that cuts something (lo > 0) runs the unwindowed kernels over the store viewed from
 * row lo, planned for T - lo tokens; lo == 0 (W >= T + 1 with k_new) is exactly the unwindowed call. Its workspace is
 * kvq_decode_attn_workspace of the attended count T - lo, which is NOT monotone in T: kvq_decode_attn_workspace_cap(dims)
 * always covers it. Device-count decode plans for min(dims->T, W - 1) tokens, so it too needs the size of that count,
 * which kvq_decode_attn_workspace_cap(dims) always covers. A window that cuts nothing in
 * extend (W >= T + S) takes exactly kvq_extend_attn's kernels; otherwise extend_attn_window_k, whose workspace fits in
 * kvq_extend_attn_workspace of the unwindowed dims (that size is non-decreasing in T), which is what the call checks. */
int kvq_decode_attn_window(const void* q, int64_t q_stride_b, int64_t q_stride_h,
                           const uint8_t* k_store, const kvq_strides_t* k_st, const float* k_scales, int k_bits,
                           const uint8_t* v_store, const kvq_strides_t* v_st, const float* v_scales, int v_bits,
                           const void* k_new, int64_t kn_stride_b, int64_t kn_stride_h,
                           const void* v_new, int64_t vn_stride_b, int64_t vn_stride_h,
                           void* out, int64_t out_stride_b, int64_t out_stride_h, int dtype, float sm_scale, int64_t window,
                           float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* dims, void* stream);
int kvq_decode_step_window(const void* q, int64_t q_stride_b, int64_t q_stride_h,
                           const void* k_new, int64_t kn_stride_b, int64_t kn_stride_h,
                           const void* v_new, int64_t vn_stride_b, int64_t vn_stride_h,
                           uint8_t* k_store, const kvq_strides_t* k_st, float* k_scales, int k_bits,
                           uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales, int v_bits,
                           void* out, int64_t out_stride_b, int64_t out_stride_h, int dtype, float sm_scale, int64_t window,
                           float eps, float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* dims, void* stream);
int kvq_decode_step_dev_window(const void* q, int64_t q_stride_b, int64_t q_stride_h,
                               const void* k_new, int64_t kn_stride_b, int64_t kn_stride_h,
                               const void* v_new, int64_t vn_stride_b, int64_t vn_stride_h,
                               uint8_t* k_store, const kvq_strides_t* k_st, float* k_scales, int k_bits,
                               uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales, int v_bits,
                               void* out, int64_t out_stride_b, int64_t out_stride_h, int dtype, float sm_scale, int64_t window,
                               float eps, float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* dims,
                               const int32_t* t_dev, void* stream);
int kvq_extend_attn_window(const void* q, int64_t q_stride_b, int64_t q_stride_h, int64_t q_stride_s,
                           const uint8_t* k_store, const kvq_strides_t* k_st, const float* k_scales, int k_bits,
                           const uint8_t* v_store, const kvq_strides_t* v_st, const float* v_scales, int v_bits,
                           const void* k_new, int64_t kn_stride_b, int64_t kn_stride_h, int64_t kn_stride_s,
                           const void* v_new, int64_t vn_stride_b, int64_t vn_stride_h, int64_t vn_stride_s,
                           void* out, int64_t out_stride_b, int64_t out_stride_h, int64_t out_stride_s, int dtype,
                           float sm_scale, int64_t window, float* workspace, int64_t workspace_floats,
                           const kvq_extend_dims_t* dims, void* stream);

/* Left-padded batches: a per-row key start. Each entry point takes the arguments of its `_window` counterpart plus
 * `kv_start` directly after `window`: a DEVICE array of dims->B int32. Key positions k < kv_start[b] of batch row b are padding:
 * a query of row b at absolute position p sees key k iff
 *     max(kv_start[b], W > 0 ? p - W + 1 : 0) <= k <= p
 * with p and W as for the `_window` calls (decode: p = T with k_new, T - 1 without; extend: p = T + s; W = window, 0 = none).
 * The host never reads kv_start (no synchronisation; a captured graph replays with the same pointer). Values out of range are
 * clamped in the kernels (negative -> 0, above the live count -> the live count; extend: above T + S -> T + S): a bad value can
 * make a result wrong, never an access out of bounds, the rule *t_dev follows. A query row that sees NO key (decode without k_new
 * and kv_start[b] >= T; an extend row whose own position is padding, T + s < kv_start[b]) writes zeros. The new token of
 * kvq_decode_step_padded / kvq_decode_step_dev_padded is always visible and is quantised into slot T (*t_dev) exactly as by
 * kvq_decode_step: kv_start never changes what is stored (the scale of a slot is shared by all batch rows).
 * kv_start == NULL is exactly the `_window` call (same kernels, same bits). Validation as for the `_window` calls, and kv_start
 * must live on the current device (KVQ_E_DEVICE).
 * CONTRACT: stored tokens of row b before kv_start[b] (and before the window's bound), and the extend chunk's k_new / v_new
 * before it, are never read, neither codes nor values; scale slots that no row needs are never read either.
 * The grid and the workspace are planned for the unpadded T (and W): kvq_decode_attn_workspace_cap(dims) / kvq_extend_attn_workspace(dims)
 * of the unpadded dims are sufficient. Workgroups whose share of row b is empty at its start exit before they request anything.
 * Kernels: every route of the unpadded plan has a padded form (decode_attn_lds_mfma_padded_k, decode_attn_partial_mfma_padded_k,
 * decode_attn_partial_padded_k; decode_attn_merge_fast_padded_k, decode_attn_merge_padded_k; extend_attn_padded_k,
 * extend_attn_merge_padded_k) that derives each row's first visible token on the device; the unpadded kernels are untouched.
 * COST: a host-count padded call has no host-side lower bound, so it runs the device-derived split layout of
 * kvq_decode_step_dev. Measured (Llama-3-8B layer, medians of six runs): all-zero starts cost the unpadded step,
 * 41.6 us per call against 42.0 (kvq_decode_step) and 42.1 (kvq_decode_step_dev) at batch 8 x 16 K tokens, 52.1 / 52.5 against
 * 52.6 / 52.3 at batch 64 x 2 K; starts uniform in [0, T/2] 35.4-36.2 us at batch 8. kvq_extend_attn_padded runs a copy of
 * extend_attn_window_k and costs what that kernel costs: 2,782 us with all-zero starts against 2,802 (kvq_extend_attn_window)
 * and 2,459 (kvq_extend_attn) at batch 4, T = 16 K, S = 512: pass NULL for a batch without padding.
 * kvq_decode_step_layers has no padded form (it has no windowed form either). */
int kvq_decode_attn_padded(const void* q, int64_t q_stride_b, int64_t q_stride_h,
                           const uint8_t* k_store, const kvq_strides_t* k_st, const float* k_scales, int k_bits,
                           const uint8_t* v_store, const kvq_strides_t* v_st, const float* v_scales, int v_bits,
                           const void* k_new, int64_t kn_stride_b, int64_t kn_stride_h,
                           const void* v_new, int64_t vn_stride_b, int64_t vn_stride_h,
                           void* out, int64_t out_stride_b, int64_t out_stride_h, int dtype, float sm_scale, int64_t window,
                           const int32_t* kv_start,
                           float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* dims, void* stream);
int kvq_decode_step_padded(const void* q, int64_t q_stride_b, int64_t q_stride_h,
                           const void* k_new, int64_t kn_stride_b, int64_t kn_stride_h,
                           const void* v_new, int64_t vn_stride_b, int64_t vn_stride_h,
                           uint8_t* k_store, const kvq_strides_t* k_st, float* k_scales, int k_bits,
                           uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales, int v_bits,
                           void* out, int64_t out_stride_b, int64_t out_stride_h, int dtype, float sm_scale, int64_t window,
                           const int32_t* kv_start,
                           float eps, float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* dims, void* stream);
int kvq_decode_step_dev_padded(const void* q, int64_t q_stride_b, int64_t q_stride_h,
                               const void* k_new, int64_t kn_stride_b, int64_t kn_stride_h,
                               const void* v_new, int64_t vn_stride_b, int64_t vn_stride_h,
                               uint8_t* k_store, const kvq_strides_t* k_st, float* k_scales, int k_bits,
                               uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales, int v_bits,
                               void* out, int64_t out_stride_b, int64_t out_stride_h, int dtype, float sm_scale, int64_t window,
                               const int32_t* kv_start,
                               float eps, float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* dims,
                               const int32_t* t_dev, void* stream);
int kvq_extend_attn_padded(const void* q, int64_t q_stride_b, int64_t q_stride_h, int64_t q_stride_s,
                           const uint8_t* k_store, const kvq_strides_t* k_st, const float* k_scales, int k_bits,
                           const uint8_t* v_store, const kvq_strides_t* v_st, const float* v_scales, int v_bits,
                           const void* k_new, int64_t kn_stride_b, int64_t kn_stride_h, int64_t kn_stride_s,
                           const void* v_new, int64_t vn_stride_b, int64_t vn_stride_h, int64_t vn_stride_s,
                           void* out, int64_t out_stride_b, int64_t out_stride_h, int64_t out_stride_s, int dtype,
                           float sm_scale, int64_t window,
                           const int32_t* kv_start, float* workspace, int64_t workspace_floats,
                           const kvq_extend_dims_t* dims, void* stream);

/* Score modifiers: logit soft-capping (Gemma 2) and per-head attention sinks (gpt-oss). One options record instead of another
 * suffix per feature; each `_ex` entry point takes the arguments of its `_padded` counterpart with `const kvq_attn_opts_t* opts`
 * in place of `window, kv_start`.
 *   window, kv_start  as for the `_padded` calls (0 / NULL = none)
 *   softcap  c > 0: every scaled score s (sm_scale * k_scales[t] * q . k_int[t] for a stored token, sm_scale * q . k_new[j] for
 *            the decode new token and the extend chunk tokens) becomes c * tanh(s / c), before masking and softmax. 0 = none.
 *   sinks    DEVICE array of dims->Hq fp32: one more softmax term per query head WITHOUT a value row,
 *            M = max(M, sinks[h]), l += exp(sinks[h] - M); the output is otherwise unchanged. NULL = none. The host never reads it
 *            (no synchronisation; a captured graph replays with the same pointer). A query row that sees no key still writes
 *            zeros: with a sink by arithmetic (acc = 0, l = 1), without one by the `_padded` rule.
 * CONTRACT: with softcap == 0 and sinks == NULL the call IS the `_padded` call (hence the `_window` or plain one when kv_start is
 * NULL or window 0): same kernels in kvq_kernel_log, same bits. opts == NULL: KVQ_E_NULL. A negative, NaN or infinite softcap:
 * KVQ_E_DIMS. sinks on another device: KVQ_E_DEVICE. Workspace sizes are unchanged (kvq_decode_attn_workspace_cap /
 * kvq_extend_attn_workspace). Every other entry point keeps its kernels and its bits.
 * Kernels (all new instantiations, suffix _mod_k; the shipped ones are untouched):
 *   soft cap  one capped form per partial family, built from the family's padded text with a NULL kv_start read as 0, so it serves
 *             plain, windowed, device-count and padded calls alike: decode_attn_lds_mfma_mod_k, decode_attn_partial_mfma_mod_k,
 *             decode_attn_partial_mod_k. tanh(x) = 1 - 2 / (2^(2 log2(e) x) + 1): one v_exp_f32 and one v_rcp_f32 per score.
 *   sinks and the capped new-token score  the merges: decode_attn_merge_fast_mod_k / _padded_mod_k, decode_attn_merge_mod_k /
 *             _padded_mod_k. A sinks-only call keeps the tuned partial kernels of the call it would be without them.
 *   extend    extend_attn_mod_k (the padded text; cap and sink of the single-split output) and extend_attn_merge_mod_k (the sink,
 *             once, when the launch has several splits).
 * Cost and register counts: DESIGN.md 3.8.
 * kvq_decode_step_layers has no `_ex` form (it has no windowed or padded one either): loop kvq_decode_step_ex over the layers. */
typedef struct {
  int64_t window;          /* keys a query sees, 0 = all */
  const int32_t* kv_start; /* device [B], NULL = none */
  float softcap;           /* 0 = none */
  const float* sinks;      /* device [Hq], NULL = none */
} kvq_attn_opts_t;
int kvq_decode_attn_ex(const void* q, int64_t q_stride_b, int64_t q_stride_h,
                       const uint8_t* k_store, const kvq_strides_t* k_st, const float* k_scales, int k_bits,
                       const uint8_t* v_store, const kvq_strides_t* v_st, const float* v_scales, int v_bits,
                       const void* k_new, int64_t kn_stride_b, int64_t kn_stride_h,
                       const void* v_new, int64_t vn_stride_b, int64_t vn_stride_h,
                       void* out, int64_t out_stride_b, int64_t out_stride_h, int dtype, float sm_scale,
                       const kvq_attn_opts_t* opts,
                       float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* dims, void* stream);
int kvq_decode_step_ex(const void* q, int64_t q_stride_b, int64_t q_stride_h,
                       const void* k_new, int64_t kn_stride_b, int64_t kn_stride_h,
                       const void* v_new, int64_t vn_stride_b, int64_t vn_stride_h,
                       uint8_t* k_store, const kvq_strides_t* k_st, float* k_scales, int k_bits,
                       uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales, int v_bits,
                       void* out, int64_t out_stride_b, int64_t out_stride_h, int dtype, float sm_scale,
                       const kvq_attn_opts_t* opts,
                       float eps, float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* dims, void* stream);
int kvq_decode_step_dev_ex(const void* q, int64_t q_stride_b, int64_t q_stride_h,
                           const void* k_new, int64_t kn_stride_b, int64_t kn_stride_h,
                           const void* v_new, int64_t vn_stride_b, int64_t vn_stride_h,
                           uint8_t* k_store, const kvq_strides_t* k_st, float* k_scales, int k_bits,
                           uint8_t* v_store, const kvq_strides_t* v_st, float* v_scales, int v_bits,
                           void* out, int64_t out_stride_b, int64_t out_stride_h, int dtype, float sm_scale,
                           const kvq_attn_opts_t* opts,
                           float eps, float* workspace, int64_t workspace_floats, const kvq_attn_dims_t* dims,
                           const int32_t* t_dev, void* stream);
int kvq_extend_attn_ex(const void* q, int64_t q_stride_b, int64_t q_stride_h, int64_t q_stride_s,
                       const uint8_t* k_store, const kvq_strides_t* k_st, const float* k_scales, int k_bits,
                       const uint8_t* v_store, const kvq_strides_t* v_st, const float* v_scales, int v_bits,
                       const void* k_new, int64_t kn_stride_b, int64_t kn_stride_h, int64_t kn_stride_s,
                       const void* v_new, int64_t vn_stride_b, int64_t vn_stride_h, int64_t vn_stride_s,
                       void* out, int64_t out_stride_b, int64_t out_stride_h, int64_t out_stride_s, int dtype,
                       float sm_scale, const kvq_attn_opts_t* opts, float* workspace, int64_t workspace_floats,
                       const kvq_extend_dims_t* dims, void* stream);

/* ---- attention mass per stored key (attention-guided eviction: H2O, SnapKV) ------------------------------------------ */

/* Workspace floats kvq_key_scores needs for these dims (-1 on bad dims; always >= 1). Non-decreasing in T for fixed B, Hq, Hkv,
 * S, D: a size taken at the store's capacity covers every shorter context. */
int64_t kvq_key_scores_workspace(const kvq_extend_dims_t* dims);

/* How much attention every stored key of one layer receives, straight from the quantised store: no fp16 copy of K, no
 * [B, Hq, S, T] score tensor. dims->T is the number of stored tokens; the S query rows are the queries OF THE LAST S STORED
 * TOKENS: row s sits at position T - S + s and sees the stored keys t <= T - S + s (causal, lower-right aligned; the window's
 * own keys come from the store). S = 1 is a decode query after its token was appended. For query head h with kv head
 * hk = h / (Hq/Hkv):
 *   sc[h,s,t]     = sm_scale * k_scales[t] * sum_d q[b,h,s,d] * k_int[b,hk,t,d]
 *   p[h,s,.]      = softmax of sc over the visible t
 *   mass[b,hk,t] (= or +=) sum over the heads h of hk's group, over the rows s that see t, of p[h,s,t]
 * so that sum_t mass[b,hk,.] = (Hq/Hkv) * S. q: [B, Hq, S, D] of `dtype` (KVQ_F16 | KVQ_BF16) laid out as for kvq_extend_attn
 * (element strides (b, h, s), D contiguous, 16-byte aligned rows, every stride a multiple of 8 elements: HF's [B, S, H, D]
 * projection passes without a copy). k_store / k_st / k_scales / k_bits as for kvq_decode_attn (8, or 4 with the even element in
 * the high nibble). mass: fp32 [B, Hkv, >= T], t contiguous, element strides (mass_stride_b, mass_stride_h) of at least T;
 * accumulate != 0 adds to what is there, one fp32 add per element (H2O's running sum over decode steps, a sum over layers).
 * Arithmetic: the exact code x scale values (the dequantised key is NOT rounded to `dtype`, as in kvq_extend_attn), fp32
 * accumulation in a fixed order: no float atomics, every mass element has one owner.
 * CONTRACT: results are bit-identical from run to run; codes and scales at slots >= T are never read; mass[.., t >= T] is never
 * written; the workspace needs no initialisation.
 * Accepted: D in {64, 128}; k_bits in {4, 8}; dtype fp16 or bf16; Hq % Hkv == 0, Hq/Hkv <= 16; 1 <= S <= T (S < 2^24,
 * T < 2^31 - 64); B * Hkv < 65536. Anything else returns KVQ_E_DIMS (KVQ_E_DTYPE for the dtype) before any launch, with an error
 * string; NULL q / k_store / k_st / k_scales / mass / workspace / dims: KVQ_E_NULL; mass on another device: KVQ_E_DEVICE.
 * NOT in this call: a sliding window, kv_start (left padding), a soft cap, sinks.
 * The normaliser of a row is known only after its whole key range has been scored, so the store is read twice (K is 1 or 0.5 byte
 * per element: cheaper than parking [rows, T] fp32 scores). Kernels: key_scores_stats_k (pass 1: the extend kernel's tile recipe,
 * only the running (m, l) of each row and split survive; a single split writes the row's log-sum-exp itself), key_scores_lse_k
 * (several splits: their log-sum-exp merge, one thread per row) and key_scores_mass_k (pass 2: one workgroup owns a run of token
 * tiles of one (batch row, kv head), walks all of the kv head's query blocks over it, and stores or accumulates its mass
 * elements). Tiles in the future of every row of a block are skipped. Design, limits and measurements: DESIGN.md 3.3.2. */
int kvq_key_scores(const void* q, int64_t q_stride_b, int64_t q_stride_h, int64_t q_stride_s,
                   const uint8_t* k_store, const kvq_strides_t* k_st, const float* k_scales, int k_bits,
                   float* mass, int64_t mass_stride_b, int64_t mass_stride_h, int accumulate,
                   int dtype, float sm_scale, float* workspace, int64_t workspace_floats,
                   const kvq_extend_dims_t* dims, void* stream);

/* Measurement aid: the NEXT kernel launch of the calling thread — whichever entry point makes it — binds these two
 * hipEvent_t (already created; either may be NULL) to its own dispatch (hipExtLaunchKernelGGL): stop - start is then
 * the kernel's duration as a profiler sees it, without the queue gaps two hipEventRecord calls around the launch
 * include. One-shot (the launch takes them). A library call that returns an error disarms the pair (no later launch
 * of the thread can take the events of a call that failed); kvq_time_next_launch(NULL, NULL) disarms a pair no launch
 * took — a call that succeeds WITHOUT launching (empty dims) or fails before it reaches the library leaves it armed, so a
 * careful caller still does that (the Python binding does, in a finally). kvq_timing_armed(): 1 while a pair is pending. */
int kvq_time_next_launch(void* start_event, void* stop_event);
int kvq_timing_armed(void);

/* Measurement aid: which kernels ran. Every launch of the calling thread notes its kernel; kvq_kernel_log writes the
 * distinct kernels launched since kvq_kernel_log_clear(), in first-launch order, one demangled name per line (what
 * rocprofv3 --kernel-trace prints) into buf (n bytes, NUL-terminated, truncated to fit) and returns their count.
 * bench.py labels every `roofline.kernel` with this, never with a name typed by hand. */
void kvq_kernel_log_clear(void);
int64_t kvq_kernel_log(char* buf, int64_t n);

/* ---- tuning knobs ---------------------------------------------------------------------------- */

/* Test knobs: each routes a call to shipped code it would not take by size or shape; results never change.
 *   "quant_force_two_pass" (0/1: generic two-pass quantise), "quant_direct_stores" (0/1: no LDS-staged stores in the
 *   256-thread quantise kernel), "quant_tile" (1 = compile-time one-wave tile kernel where the shape has one, default;
 *   0 = general kernels), "quant_wide" (1 = single-pass 1024-thread register tile for batched slices of 16384 < B*H*D <=
 *   131072 two-byte elements, default; 0 = split phases / swept tile), "quant_block" (general quantise kernel: 64 =
 *   one-wave tiles, default; anything else = 256 threads), "quant_few_tokens" (kvq_absmax_tokens on slices of at most
 *   this many tokens: one workgroup per (group, token) and a plain store; 0 = always the tile walk's atomics),
 *   "pool_wave" (1 = one wave per output row where the shape allows, default; 0 = per-lane-group walk), "gather_rows"
 *   (token gather: 1 = 4 KiB work items, one 16-byte piece per thread, default; 0 = the grid-stride kernel),
 *   "store_pool_fast" (kvq_store_chunk_pool: 1 = the register kernel where the layout allows, default; 0 = the generic
 *   kernel),
 *   "attn_force_valu" (0/1), "attn_stream_tpw" (tiles per wave of the ring attention kernel: -1 never, 0 by size, > 0
 *   that many), "attn_lds" (the LDS-staged ring kernel: -1 by shape, default; 0 never), "attn_ring_dev"
 *   (kvq_decode_step_dev on the ring kernel where the host-side call takes it: 1, default; 0 = always one-tile splits),
 *   "attn_merge_wave" (merge of <= 16 splits at head_dim 128: 1 = one wave per head, default; 0 = one workgroup per
 *   head), "attn_merge_fast" (1 = the merge that requests everything up front where it applies, default; 0 = the
 *   chained merge, which serves more than 256 splits), "attn_new_token_parts" (kvq_decode_step with a new-token slice
 *   past 8,192 elements: 1 = one workgroup per 8,192 elements, default; 0 = the generic one-workgroup routine).
 * Returns 0, or KVQ_E_DIMS for an unknown key; kvq_get_tunable returns 0 for one. Process-global. */
int kvq_set_tunable(const char* key, int64_t value);
int64_t kvq_get_tunable(const char* key);

#ifdef __cplusplus
}
#endif
#endif /* KVQ_HIP_H */

/* pianobart_hip.h -- C ABI of libpianobart_hip.so (gfx950 / MI355X).
 *
 * The reference (RS2002/PianoBart) has no FFI: its hot path is Python calling ATen ops through
 * `transformers.BartModel`. This header is the boundary a maintainer binds
 * instead (ctypes stub in INTEGRATION.md): one entry per op of SURVEY.md 2.2, plain pointers and
 * sizes, a hipStream_t passed as void*, int status (0 = ok; otherwise pb_last_error() describes it).
 * All pointers are DEVICE pointers unless stated. No global state besides the last-error string.
 *
 * Storage dtype of activations / weight shadows: PB_F32 (exact-f32 parity path, f32-input MFMA)
 * or PB_BF16 (throughput path, bf16 MFMA, f32 accumulate). Statistics, loss, optimizer state,
 * biases and LayerNorm parameters are always f32.
 */
#ifndef PIANOBART_HIP_H
#define PIANOBART_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PB_F32 0
#define PB_BF16 1
#define PB_F32X3 2   /* pb_gemm only (ABI 8): f32 operands, f32 C and aux, the products as split-bf16 triples a_hi b_hi + a_hi b_lo + a_lo b_hi on the
                        bf16 matrix cores with f32 accumulation (~2^-16 relative per product): the parity-grade instantiation that is not bound by
                        the f32-input MFMA rate (precision="bf16x3"); every other op of that instantiation runs its PB_F32 form */

#define PB_ABI_VERSION 10  /* 10: pb_attn_desc + pb_attn_fwd / pb_attn_bwd / pb_attn_desc_bytes (the ten pb_flash_fwd* / pb_flash_bwd* calls removed); 9: one fused decoder for every B (pb_batch_decoder_*, + pb_batch_decoder_step; pb_decoder_* removed); 8 (round 6): + pb_decoder_sampler_init / launch / wait / logs / seek (device-sampled decode), dtype PB_F32X3 in pb_gemm, pb_flash_*_x3, pb_gemm_reserve_cus; 7 (round 5): + PB_GEMM_ROWDOT / rowdot_out in pb_gemm_desc, delta_rows in pb_flash_bwd1*; 6 (round 5): + pb_flash_bwd1_supported; 5 (round 4): + pb_flash_bwd1*, bh_order in the packed attention calls; 4 (round 3): + pb_decoder_*, pb_nucleus_rows, pb_ids_check */
int pb_abi_version(void);
const char* pb_last_error(void);

/* ---- K3/K5/K6/K7/K8 (+ unfused attention products): C (+)= epi(alpha * A.B^T) ------------------
 * Replaces nn.Linear forward/backward inside transformers BartAttention / Bart*Layer
 * (modeling_bart.py:207,227-228,255,297-302) and model.py:124-125 (MLM heads); PianoBart.py:68,71.
 * A(m,k): a_kcontig ? A[m*lda + k] : A[k*lda + m];  B(n,k): b_kcontig ? B[n*ldb + k] : B[k*ldb + n].
 * Batched over nb1*nb2 problems with element strides s?1 / s?2. */
#define PB_GEMM_ACCUM 1          /* C = C + result                                   */
#define PB_GEMM_C_F32 2          /* C is float regardless of dtype                   */
#define PB_GEMM_GELU 4           /* C = gelu_erf(result); aux_out = gelu_erf'(result): the forward pays 3 extra FMAs per element so that */
#define PB_GEMM_MUL_GELU_GRAD 8  /* C = result * aux_in      ... the backward of the activation (dU = dG * gelu'(U)) is one multiply        */
#define PB_GEMM_FORCE_V1 16      /* use the generic register-staged kernel (tests)    */
#define PB_GEMM_TILE128 32       /* bf16 fast path: force the 128x128 tile             */
#define PB_GEMM_TILE256 64       /* bf16 fast path: prefer the 256x256 tile (default when M >= 2048, N >= 512, no split-K) */
#define PB_GEMM_NO_EPILOGUE 128  /* profiling: main loop only, nothing is stored                                    */
#define PB_GEMM_REG_EPILOGUE 256 /* A/B runs: interior tiles of the 256x256 kernel store straight from the MFMA register layout (64-byte row pieces on
                                    lanes 16 apart) instead of through the row staging (8 rows x 128 contiguous bytes per instruction)            */
#define PB_GEMM_ONE_BARRIER 2048 /* A/B runs: 256x256 tile with the one-barrier kernel instead of the ping-pong one   */
#define PB_GEMM_PLAIN_GRID 4096  /* 256x256 ping-pong kernel as an ordinary grid (one workgroup per work item) instead of the
                                    persistent one-per-CU grid: what to ask for when other kernels (RCCL) hold CUs        */
#define PB_GEMM_TAIL_SPLIT 32768 /* 256x256 kernel: the tiles of a partly filled last round of the grid may be cut into K ranges that
                                    occupy the idle CUs (f32 partials, finished by a second small launch); a cost model decides.
                                    Pays for a caller that runs one GEMM at a time (N = 768 at 26 624 rows: +13-17 %): the training
                                    step asks for it in forward; in backward its second stream already fills those CUs     */
#define PB_GEMM_ROWDOT 131072     /* C = result as usual, and per 64-column group the row sums of C * aux_in go to rowdot_out (see pb_gemm_desc) */
#define PB_GEMM_LEAVE_CUS 262144  /* persistent grids: launch CUs - pb_gemm_reserve_cus() workgroups instead of one per CU (data parallel: the backward
                                    GEMMs that run beside RCCL's resident kernels)                                                       */
#define PB_GEMM_ROW_SPLIT 65536  /* 256x256 kernel: the M tiles of the full rounds of the persistent grid stay with it, the remaining rows go to a
                                    second launch of the 128x128 kernel (no partials). Measured (round 3): -1.8 % on the one-stream step
                                    together with nothing else, +-0 on the shipped two-stream step (its second stream already fills the CUs a
                                    short last round leaves idle, and the forward's K = 768 shapes lose what the split saves to the slower
                                    128x128 tiles): on request only                                                                   */
typedef struct pb_gemm_desc {
    const void* A; const void* B; void* C;
    const float* bias;            /* per-n, may be NULL */
    const void* aux_in; void* aux_out; /* dtype storage, leading dim ldaux */
    int32_t dtype, a_kcontig, b_kcontig, flags;
    int32_t M, N, K, nb1, nb2, _pad;
    int64_t lda, ldb, ldc, ldaux;
    int64_t sA1, sA2, sB1, sB2, sC1, sC2;
    float alpha; float _pad2;
    int32_t splitk; int32_t _pad3;   /* >1: split K over blockIdx.z into f32 slabs (bf16, f32 C, no epilogue) */
    void* slabs;                      /* workspace of splitk*M*N floats when splitk > 1 */
    float* colsum_out;                /* optional: colsum_out[n] += sum_m C[m][n] (the bias gradient of the layer that produced C's
                                         cotangent, e.g. db1 from dU): taken from the epilogue registers of the 256x256 kernel, by a
                                         pb_colsum pass over C otherwise. Needs colsum_ws; single batch, no split-K, ldc == N, N % 4 == 0 */
    float* colsum_ws;                 /* workspace of pb_gemm_colsum_ws_floats(M, N) floats */
    float* rowdot_out; int64_t ld_rowdot; /* PB_GEMM_ROWDOT (ABI 7): rowdot_out[(n / 64) * ld_rowdot + m] = sum over columns 64 (n / 64) .. + 63 of
                                         bf16(C[m][.]) * aux_in[m][.], f32 -- with C = dO (the input gradient of the attention output
                                         projection) and aux_in = O this is the delta = rowsum(dO * O) per head that the one-pass pb_attn_bwd reads
                                         (delta_rows). NT layout, M and N multiples of 256, bf16, no other epilogue; refused otherwise */
} pb_gemm_desc;
int pb_gemm(const pb_gemm_desc* d, void* stream);
/* CUs (rounded up to a multiple of 8) that the persistent one-workgroup-per-CU GEMM grids launched with PB_GEMM_LEAVE_CUS leave to other resident kernels -- RCCL's, in a
 * data-parallel job (the reference: nn.DataParallel's reduce_add on the side, pretrain.py:63-65). Process-wide; 0 = none (default). ABI 8. */
int pb_gemm_reserve_cus(int32_t n);
int64_t pb_gemm_colsum_ws_floats(int32_t M, int32_t N);

/* ---- K1/K2: Octuple gather-sum + position + LayerNorm (+dropout) -----------------------------
 * Replaces PianoBart.py:60-71 (8 x Embedding*16 -> cat -> Linear) and modeling_bart.py:520-525 /
 * 648-654 (x + pos[s+2] -> layernorm_embedding -> dropout). P is the projected table
 * P[off_i + v] = 16 * E_i[v] @ W_lin[:, 256 i : 256 i + 256]^T  (1280 x d, f32), built with pb_gemm. */
int pb_ids_to_i16(const int64_t* ids, int16_t* out, int64_t n, void* stream);
/* Range check of (T,8) Octuple ids against the 8 table sizes (device int32[8], classes order): *flag |= 1 (device word) when an id is
 * negative or >= its table size -- what nn.Embedding answers with an IndexError (PianoBart.py:15-16). pb_ids_to_i16 writes -1
 * for a value that does not fit int16, so a checked conversion cannot alias into a valid id. An offending id is REPLACED by 0 in
 * ids16, so that the gather kernels enqueued behind the check never leave their tables; the host reads the word at its next
 * synchronisation point (Engine.check_ids) and raises before any result is used. */
int pb_ids_check(int16_t* ids16, int64_t n, const int32_t* limits8, int32_t* flag, void* stream);
int pb_embed_ln_fwd(const int16_t* ids16 /*(T,8)*/, const float* P, const int32_t* seg_off /*host, 8*/,
                    const float* lin_bias, const float* pos /*(S+2,d)*/, const float* ln_w, const float* ln_b,
                    void* y /*(T,d) dtype*/, float* mean, float* rstd, int32_t T, int32_t S, int32_t d,
                    int32_t dtype, float eps, uint64_t seed, uint32_t site, float p_drop, void* stream);
/* backward: dy -> dbias (d), dgamma/dbeta (d) and either (dz_out == NULL) dP / dpos by f32 atomic scatter-add
 * (exact-f32 path), or (dz_out != NULL) dz (T,d) in dtype for the atomic-free route:
 * dP = Onehot^T dz through pb_gemm (pb_onehot_build) and dpos through pb_batch_sum. */
int pb_embed_ln_bwd(const void* dy, const int16_t* ids16, const float* P, const int32_t* seg_off,
                    const float* lin_bias, const float* pos, const float* ln_w, const float* mean,
                    const float* rstd, float* dP, float* dpos, float* dbias, float* dgamma, float* dbeta,
                    float* partials /*workspace, pb_ln_partials_floats()*/, void* dz_out, int32_t T, int32_t S, int32_t d,
                    int32_t dtype, uint64_t seed, uint32_t site, float p_drop, void* stream);
/* the same two on packed rows (pb_rowmap_build): row r is row row_ids[r] = b*S + s of the padded batch, i.e. it sits at sequence
 * position row_ids[r] % S and draws the dropout bits of that row (a packed step drops exactly what the padded step drops);
 * T need not be a multiple of S. With dz_out the position-table gradient comes from pb_pos_grad_packed. */
int pb_embed_ln_fwd_packed(const int16_t* ids16, const int32_t* row_ids, const float* P, const int32_t* seg_off,
                           const float* lin_bias, const float* pos, const float* ln_w, const float* ln_b, void* y,
                           float* mean, float* rstd, int32_t T, int32_t S, int32_t d, int32_t dtype, float eps,
                           uint64_t seed, uint32_t site, float p_drop, void* stream);
int pb_embed_ln_bwd_packed(const void* dy, const int16_t* ids16, const int32_t* row_ids, const float* P,
                           const int32_t* seg_off, const float* lin_bias, const float* pos, const float* ln_w,
                           const float* mean, const float* rstd, float* dP, float* dpos, float* dbias, float* dgamma,
                           float* dbeta, float* partials, void* dz_out, int32_t T, int32_t S, int32_t d, int32_t dtype,
                           uint64_t seed, uint32_t site, float p_drop, void* stream);
/* onehot (T,V) bf16 with ones at columns seg_off[i] + ids16[t][i] */
int pb_onehot_build(const int16_t* ids16, const int32_t* seg_off /*host 8*/, void* out, int64_t T, int32_t V, void* stream);
/* out[i] += sum_b x[b*Sd + i], i < Sd */
int pb_batch_sum(const void* x, float* out, int32_t B, int64_t Sd, int32_t dtype, void* stream);

/* ---- K5/K6 tail: y = LayerNorm(res + dropout(a)) ------------------------------------------------
 * Replaces dropout + residual + LayerNorm of modeling_bart.py:292-294,300-302,362-364,377-379,386-388. */
int64_t pb_ln_partials_floats(int32_t d);
int pb_add_ln_fwd(const void* res, const void* a, const float* ln_w, const float* ln_b, void* y,
                  float* mean, float* rstd, int32_t T, int32_t d, int32_t dtype, float eps,
                  uint64_t seed, uint32_t site, float p_drop, void* stream);
/* on packed rows: row r draws the dropout bits of row row_ids[r] of the padded batch */
int pb_add_ln_fwd_packed(const void* res, const void* a, const float* ln_w, const float* ln_b, void* y,
                         float* mean, float* rstd, const int32_t* row_ids, int32_t T, int32_t d, int32_t dtype, float eps,
                         uint64_t seed, uint32_t site, float p_drop, void* stream);
/* dres gets dz (accumulated into if accum_dres), da gets dz*dropmask; dgamma/dbeta/dbias_a are ADDED to. */
int pb_add_ln_bwd(const void* dy, const void* res, const void* a, const float* ln_w, const float* mean,
                  const float* rstd, void* dres, void* da, float* dgamma, float* dbeta, float* dbias_a,
                  float* partials, int32_t T, int32_t d, int32_t dtype, int32_t dres_f32, int32_t accum_dres,
                  uint64_t seed, uint32_t site, float p_drop, void* stream);
int pb_add_ln_bwd_packed(const void* dy, const void* res, const void* a, const float* ln_w, const float* mean,
                         const float* rstd, void* dres, void* da, float* dgamma, float* dbeta, float* dbias_a,
                         float* partials, const int32_t* row_ids, int32_t T, int32_t d, int32_t dtype, int32_t dres_f32,
                         int32_t accum_dres, uint64_t seed, uint32_t site, float p_drop, void* stream);

/* ---- bias gradients: out[n] += sum_t dy[t][n] --------------------------------------------------*/
/* partials: workspace of at least pb_colsum_partials_floats(N) floats */
int64_t pb_colsum_partials_floats(int32_t N);
int pb_colsum(const void* dy, int64_t ld, float* out, float* partials, int32_t T, int32_t N, int32_t dtype,
              int32_t src_f32, void* stream);
/* pb_colsum for any N and ld (an addition to ABI 10; pb_colsum itself needs multiples of 4: a lane owns 4 adjacent columns): a thread
 * owns one column. The head-bias gradient of a dictionary whose vocabulary total is no multiple of 4. Same workspace, accumulates alike. */
int pb_colsum_any(const void* dy, int64_t ld, float* out, float* partials, int32_t T, int32_t N, int32_t dtype,
                  int32_t src_f32, void* stream);

/* ---- K4 (unfused form, both dtypes): masked softmax over key axis -------------------------------
 * scores (B,H,Sq,Sk) f32 = q.k^T (unscaled); P = softmax(scale*scores + mask); a query row with no
 * visible key gives an all-zero row (transformers 5.x SDPA behaviour, oracle header).
 * key_mask (B,Sk) float (!=0 keeps) or NULL; causal: key j visible to query i iff j <= i. */
int pb_softmax_fwd(const float* scores, const float* key_mask, void* P, int32_t B, int32_t H, int32_t Sq,
                   int32_t Sk, float scale, int32_t causal, int32_t dtype, void* stream);
/* dS = scale * P * (dP - rowsum(dP*P)) written in dtype */
int pb_softmax_bwd(const float* dP, const void* P, void* dS, int64_t rows, int32_t Sk, float scale,
                   int32_t dtype, void* stream);

/* ---- K4 fused: flash attention forward / backward, one descriptor for every form (ABI 10) ------------
 * Replaces modeling_bart.py:115-140 (eager) / F.scaled_dot_product_attention and its autograd backward.
 * dtype PB_BF16: q,k,v,o,dout,dq,dk,dv bf16, head_dim 32 / 64 / 96 / 128, strides multiples of 8 elements (dq_ss: of 4 for the kernel pair).
 *   head_dim 64 / 96 / 128 run the pipelined kernels (pb_flash64.hip), head_dim 32 or PB_ATTN_GENERIC the generic ones (pb_flash.hip).
 *   Backward = dQ (+ delta) and dK/dV kernels, no atomics, deterministic.
 * dtype PB_F32X3 (the "bf16x3" parity instantiation, round 6): f32 q / k / v / o / gradients, every product a split-bf16 triple on the bf16
 *   matrix cores (see PB_F32X3), softmax in f32 -- instead of the unfused QK^T -> softmax -> PV chain of the exact-f32 path, whose
 *   (B, H, S, S) f32 matrices dominate that path's HBM time. head_dim 32 / 64 / 128 (pb_flash_x3_supported), strides multiples of 4
 *   elements, operands 16-byte aligned. No dbias_*, bh_order or one-pass backward; kmax is read only beside a key_mask.
 * Element (b,s,h,c) of an operand at ptr[b*sb + s*ss + h*hd + c], strides in ELEMENTS; dout has o's strides; lse, delta: (B,H,Sq) f32
 * (delta is scratch written by the backward). Masks: key_mask (B,Sk) float (!= 0 keeps) or NULL, PB_ATTN_CAUSAL: key j visible to
 * query i iff j <= i; a query without a visible key gives a zero output row and lse = +inf.
 * kmax (B) int32, optional: 1 + index of the last visible key of each batch row (pb_key_extent); key tiles at or beyond it are skipped
 * (they are masked for every query). NULL = no skipping. Used by the pipelined and the split-bf16 kernels.
 *
 * Packed rows (dead-row compaction; bf16: head_dim 64 / 96 / 128): the PAD tail the reference computes and then masks (PianoBart.py:60-75:
 * attention_mask hides rows as keys only) is dropped: the rows of the batch lie back to back. Batch b's query rows are rows q_off[b] ..
 * q_off[b] + q_len[b] - 1 of q / o / dout / dq (row stride *_ss, element (row, h, c) at ptr[row*ss + h*hd + c]), its key rows k_off[b] ..
 * k_off[b] + k_len[b] - 1 of k / v / dk / dv; the first k_vis[b] key rows of the batch are the visible ones (the rest receive no gradient
 * and are seen by no query). Causal: key row j is visible to query row i of the same batch iff j <= i (row indices within the batch) and
 * j < k_vis[b]. The five descriptors are device int32 (B), all set or all NULL; with them Sq / Sk are the maxima of q_len / k_len (grid
 * and LDS sizing, row length of lse / delta), and key_mask, kmax and the batch strides are not read.
 * bh_order (device int32, B * H entries, or NULL): the order in which the grid takes the (batch, head) pairs (entry = b * H + h). Costs
 * spread 4x over a packed batch; a caller that lists the pairs longest first, dealt eight at a time (one per XCD), removes the tail
 * of a static grid. It changes the order of the work only: results are bit-identical with and without it. Read with packed rows only.
 *
 * dbias_q / k / v, dbias_ws (optional, all or none; pipelined kernels only): dbias_x[c] += column sums of dQ / dK / dV over (batch, position)
 * = the bias gradients of the q / k / v projections, taken from the kernels' epilogue registers; dbias_ws: pb_flash_bias_ws_floats(B, H,
 * Sq, Sk, hd) floats.
 *
 * PB_ATTN_ONE_PASS (K4b, pb_flash1.hip, bf16 head_dim 64, where pb_flash_bwd1_supported): the same backward (to bf16 rounding) computed
 * key-stationary: a workgroup owns 256 keys of one (batch, head), keeps their dK / dV in accumulator registers and sweeps the query tiles
 * once (5 matrix products and one exp pass per (query, key) pair instead of 7 and 2). dQ is summed over the key blocks without atomics:
 * block j writes its partial into bf16 slab j of dq_ws (required: pb_flash_bwd1_ws_bytes(rows of the q side, H, hd, Sk) bytes), a second
 * kernel adds a row's slabs in f32 in block order and rounds once. Deterministic. q_rows: rows of the q tensor (packed rows; dense: B * Sq
 * is used). delta_rows (may be NULL): delta = rowsum(dO * O) per head as [H][rows of the q side] (dense: row = b * Sq + s), e.g. written by
 * the PB_GEMM_ROWDOT epilogue of the GEMM that produced dO; NULL = the call computes it itself into `delta` with one more launch.
 *
 * A descriptor starts zeroed: what a call does not use stays 0 / NULL. pb_attn_fwd reads q, k, v and writes o, lse; pb_attn_bwd reads
 * q, k, v, o, dout, lse and writes dq, dk, dv, delta. Both refuse a descriptor that names a combination without kernels. */
int pb_key_extent(const float* key_mask, int32_t* kmax, int32_t B, int32_t Sk, void* stream);
#define PB_ATTN_CAUSAL 1
#define PB_ATTN_GENERIC 2        /* bf16, dense: use the generic kernels whatever the head_dim (tests); not with head_dim 96 */
#define PB_ATTN_ONE_PASS 4       /* pb_attn_bwd: the one-pass kernel; pb_attn_fwd refuses the bit where pb_attn_bwd would (dtype, head_dim, generic) and otherwise ignores it */
typedef struct pb_attn_desc {
    const void *q, *k, *v; void* o; const void* dout; void *dq, *dk, *dv; float *lse, *delta;
    const float* key_mask; const int32_t* kmax;
    const int32_t *q_off, *q_len, *k_off, *k_len, *k_vis, *bh_order;
    float *dbias_q, *dbias_k, *dbias_v, *dbias_ws;
    void* dq_ws; const float* delta_rows; int64_t q_rows;
    int64_t q_sb, q_ss, k_sb, k_ss, v_sb, v_ss, o_sb, o_ss, dq_sb, dq_ss, dk_sb, dk_ss, dv_sb, dv_ss;
    int32_t dtype, B, H, Sq, Sk, hd, flags; float scale;
} pb_attn_desc;
int pb_attn_fwd(const pb_attn_desc* d, void* stream);
int pb_attn_bwd(const pb_attn_desc* d, void* stream);
int64_t pb_attn_desc_bytes(void);
int64_t pb_flash_bias_ws_floats(int32_t B, int32_t H, int32_t Sq, int32_t Sk, int32_t hd);
int64_t pb_flash_bwd1_ws_bytes(int64_t rows, int32_t H, int32_t hd, int32_t Sk_max);
/* 1 if the one-pass kernel takes the shape (head_dim 64, Sq_max <= 6144: its per-sequence -lse / -delta tables live in LDS; dQ slabs
 * <= 8 GiB), else 0: call pb_attn_bwd without PB_ATTN_ONE_PASS. rows = rows of the q side (dense: B * Sq). */
int32_t pb_flash_bwd1_supported(int32_t Sq_max, int32_t Sk_max, int32_t hd, int64_t rows, int32_t H);
int pb_flash_x3_supported(int32_t hd);

/* ---- row maps for the packed step (pb_rowmap.hip) ------------------------------------------------
 * pb_rowmap_count: counts (B,8) int32 = {encoder rows visible as keys (emask != 0), decoder rows visible as keys (dmask != 0),
 *   decoder live rows (visible, or loss_mask (B,S,8) row != 0), 1 iff the visible decoder positions are exactly 0 .. L-1,
 *   decoder rows with a loss term, 0, 0, 0}.
 * pb_rowmap_build: batch b's packed rows off[b] .. off[b] + len[b] - 1 = its positions with mask != 0 (ascending), then those
 *   with a loss term (loss_mask may be NULL), then its first remaining (dead) positions up to len[b]; row_src[r] = b*S + s and
 *   row_pos[r] = s for packed row r, inv (B*S) = packed row of (b, s) or -1. len[b] must cover the first two classes.
 * pb_rowmap_build_sub: the rows of an existing packing (present (B*S) = its `inv`) that the LAST decoder layer's query side needs:
 *   batch b's rows off[b] .. + len[b] - 1 = its positions with a loss term (ascending), then other positions of the packing;
 *   row_src[r] = b*S + s, row_idx[r] = present[b*S + s] (the row of the existing packing). len[b] <= rows of b in that packing.
 * pb_gather_rows16: dst row r = src row row_src[r] (row_bytes a multiple of 16). pb_scatter_rows16: dst row row_dst[r] = src row r.
 * pb_pos_grad_packed: out (S,d) f32 += sum_b x[inv[b][s]] (the position-table gradient; replaces pb_batch_sum). */
int pb_rowmap_count(const float* emask, const float* dmask, const float* loss_mask, int32_t* counts, int32_t B, int32_t S,
                    void* stream);
int pb_rowmap_build(const float* mask, const float* loss_mask, const int32_t* off, const int32_t* len, int32_t* row_src,
                    int32_t* row_pos, int32_t* inv, int32_t B, int32_t S, void* stream);
int pb_rowmap_build_sub(const float* loss_mask, const int32_t* present, const int32_t* off, const int32_t* len,
                        int32_t* row_src, int32_t* row_idx, int32_t B, int32_t S, void* stream);
int pb_gather_rows16(const void* src, const int32_t* row_src, void* dst, int64_t n_rows, int32_t row_bytes, void* stream);
int pb_scatter_rows16(const void* src, const int32_t* row_dst, void* dst, int64_t n_rows, int32_t row_bytes, void* stream);
int pb_pos_grad_packed(const void* x, const int32_t* inv, float* out, int32_t B, int32_t S, int32_t d, int32_t dtype,
                       void* stream);

/* ---- K9: fused 8-segment log-softmax + CE + argmax + masked accuracy (+ dlogits) ----------------
 * Replaces pretrain.py:112-118,163-189 (np.argmax x8, CrossEntropyLoss x8, masked means).
 * logits (T,V) f32 with the 8 heads at column offsets seg_off[i]; target (T,8) int16; loss_mask
 * (T,8) f32. sums (3,8) f32 += {sum ce*m, sum m, sum correct*m}. If dlogits != NULL:
 * dlogits[t, off_i+c] = coef[i] * m[t,i] * (softmax_c - 1[c==target]) in dtype, coef (8) device f32
 * (= w_i / (sum_w * M_i)). argmax_out (T,8) int16 may be NULL. */
int pb_ce_fwd_bwd(const float* logits, const int16_t* target, const float* loss_mask, const int32_t* seg_off /*host 9*/,
                  float* sums, float* partials, const float* coef, void* dlogits, int16_t* argmax_out,
                  int32_t T, int32_t V, int32_t dtype, void* stream);
int64_t pb_ce_partials_floats(void);
/* counts[i] = sum_t loss_mask[t,i]  (f32, 8) -- the M_i of pretrain.py:117 */
int pb_mask_count(const float* loss_mask, float* counts, float* partials /* >= pb_ce_partials_floats() */, int64_t T, void* stream);
/* coef[i] = scale * w[i] / (sum_w * counts[i])   (scale = 1 for pretrain.py:185-189; finetune_generation.py:241-250 uses
 * w_i = weight_i * n_tok_i with the denominator sum(n_tok), i.e. scale = sum_w / sum(n_tok)) */
int pb_loss_coef(const float* counts, const float* w /*device 8*/, float* coef, float scale, void* stream);

/* ---- K28: K9 with soft targets: knowledge distillation and label smoothing (pb_distill.hip; additions to ABI 10) ----
 * Everything of pb_ce_fwd_bwd (logits, target, loss_mask, seg_off, coef, dlogits in dtype or NULL, argmax_out or NULL, T, V) plus
 *   teacher  (T_t,V) f32  the teacher's logits in the same layout, or NULL (then alpha must be 0 and plane 5 stays 0)
 *   t_row    (T) int32    the teacher row that student row t reads, or NULL: row t reads row t (then T_t >= T). A row number outside
 *                         0 .. T_t - 1 is not read: that row's teacher logits count as NaN
 *   alpha in [0,1], tau > 0 and finite, eps in [0,1): host scalars
 * Per row t and head i of n classes, z = the student's logits of the head, u = the teacher's of row t_row[t], y = target, m = loss mask,
 * p = softmax(z), p_tau = softmax(z / tau), q = softmax(u / tau), each softmax on its own maximum:
 *   hard   = -log p[y]                                   (a target outside its head scores a logit of 0 and has no one-hot column)
 *   hard_e = (1 - eps) hard - (eps / n) sum_c log p[c]
 *   kl     = sum_c q[c] (log q[c] - log p_tau[c])        (a class with q == 0 counts as 0), as
 *            sum_c q[c] ((u[c] - max u) - (z[c] - max z)) / tau + log sum_c e^((z[c] - max z) / tau) - log sum_c e^((u[c] - max u) / tau)
 *   loss   = (1 - alpha) hard_e + alpha tau^2 kl
 *   dlogits[t, off_i + c] = coef[i] m ((1 - alpha) (p[c] - (1 - eps) [c == y] - eps / n) + alpha tau (p_tau[c] - q[c]))
 * (d kl / dz = (p_tau - q) / tau, so the soft part carries tau, not tau^2). coef[i] * m multiplies: a head without any loss position has
 * coef = inf and NaN gradients exactly where K9 has them. argmax is the first maximum.
 * sums (5,8) f32 += {sum loss*m, sum m, sum correct*m, sum hard*m, sum kl*m}; the second and third are exact counts. Per-workgroup
 * partials (partials: >= pb_distill_partials_floats() floats) are added in a fixed order: equal inputs give equal bytes.
 * alpha = 0, eps = 0 and teacher NULL compute K9's quantities. Heads of at most 320 classes run a register-resident form (one wave64
 * holds the student's and the teacher's row), others (up to 1088 classes) one head at a time; both use the same arithmetic. */
int pb_distill_fwd_bwd(const float* logits, const float* teacher, const int32_t* t_row, const int16_t* target, const float* loss_mask,
                       const int32_t* seg_off /*host 9*/, float* sums, float* partials, const float* coef, void* dlogits,
                       int16_t* argmax_out, int32_t T, int32_t T_t, int32_t V, int32_t dtype, float alpha, float tau, float eps,
                       void* stream);
int64_t pb_distill_partials_floats(void);

/* ---- K16: teacher-forced scoring (pb_score.hip; additions to ABI 9) ---------------------------------
 * The forward-only quantity of Ablation.py:126-166 (a teacher-forced decoder pass evaluated against the piece), per token instead of
 * K9's 24 batch-wide sums. logits (T,V) f32 and seg_off as for pb_ce_fwd_bwd; target (T,8) int16; mask (T) f32 of 0 / 1, one value per
 * POSITION. Per position and head, each (T,8):
 *   logp    f32   x[target] - logsumexp(head), maximum subtracted
 *   entropy f32   -sum p log p of the head's softmax, as log(sum e) - sum e (x - max) / sum e with e = exp(x - max); p == 0 counts as 0
 *   rank    int16 columns of the head that beat the target: a greater logit, or an equal one at a lower index -- rank == 0 iff the
 *                 target is the first maximum, the argmax of pb_ce_fwd_bwd
 * A position with mask == 0 gets logp = 0, entropy = 0, rank = -1 and neither its logits nor its target are read. entropy and rank may
 * be NULL. Heads of 1 .. 1088 classes: up to 320 the register-resident row layout of K9, above it a wide form that holds one head's
 * 17 classes per lane at a time (same arithmetic and summation order); a target outside its head scores a logit of 0 as in K9.
 * The rank of such a target follows from the same rule with that logit of 0 at the target's own index: rank = #(x > 0) +
 * #(x == 0 at a column < target). So a target < 0 counts none of the head's zeros (+0.0 and -0.0 alike) and a target >= n all of
 * them; a target < 0 on a head without a positive logit has rank 0 although it is no argmax.
 * pb_seq_scores: out (B,4,8) f32 = per sequence and head {sum mask*logp, sum mask*entropy, sum mask*[rank == 0], sum mask} over the S
 * positions of sequence b (rows b*S .. b*S + S - 1 of the (B*S,8) arrays); entropy / rank NULL leave their plane 0. One workgroup per
 * sequence, fixed summation order, no atomics (bit-reproducible): per head 32 running sums, sum g over the positions g, g + 32,
 * g + 64, ... in order, then the 32 sums added in order of g. */
int pb_token_scores(const float* logits, const int16_t* target, const float* mask, const int32_t* seg_off /*host 9*/, float* logp,
                    float* entropy, int16_t* rank, int32_t T, int32_t V, void* stream);
int pb_seq_scores(const float* logp, const float* entropy, const int16_t* rank, const float* mask, float* out, int32_t B, int32_t S,
                  void* stream);

/* ---- K10/K11: global grad norm, clip, HF-AdamW, bf16 shadow refresh --------------------------------
 * Replaces clip_grad_norm_(.,3.0) (pretrain.py:195) and transformers.AdamW.step (pretrain.py:76,196;
 * 4.29.2 formula: eps added to sqrt(v) before bias correction, decoupled decay after the update). */
int64_t pb_norm_partials_floats(void);
int pb_grad_sqnorm(const float* g, int64_t n, float* partials, float* out_sq /*1 float, overwritten*/, void* stream);
/* clip_coef = min(1, max_norm / (sqrt(sq * gscale^2) + 1e-6)) * gscale */
int pb_clip_coef(const float* sq, float max_norm, float gscale, float* coef, void* stream);
int pb_adamw_step(float* p, const float* g, float* m, float* v, void* shadow /*bf16 or NULL*/, int64_t n,
                  const float* clip_coef /*device, may be NULL*/, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int32_t step, void* stream);
int pb_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
/* x (n f32, n % 8 == 0) -> hi = bf16(x), lo = bf16(x - hi): the two planes of the split-bf16 arithmetic (precision="bf16x3") as separate arrays, for products whose
 * other operand is exact in bf16 (the one-hot matrix of the embedding-table gradient: Onehot^T dz = Onehot^T dz_hi + Onehot^T dz_lo). Replaces nothing in the
 * reference: torch.nn.Embedding's backward (index_add in f32) is what the pair of GEMMs computes. */
int pb_split_bf16(const float* x, void* hi, void* lo, int64_t n, void* stream);
int pb_cast_bf16_to_f32(const void* src, float* dst, int64_t n, void* stream);
int pb_fill_f32(float* dst, float value, int64_t n, void* stream);
/* Transposed copies of the weight matrices inside the flat bf16 shadow: table (device, n_matrices x 4 int32) = {element offset, R, C,
 * index of the matrix's first 64x64 tile}; matrix e (R x C row-major at src + offset) is written C x R at dst + offset; R, C and
 * offset multiples of 8; n_tiles = sum of ceil(R/64) ceil(C/64). The backward's dX = dY W then reads W^T as a K-contiguous operand
 * (the NT form of the GEMM kernel is 7-20 % faster than the NN form). */
int pb_transpose_batch_bf16(const void* src, void* dst, const int32_t* table, int32_t n_matrices, int32_t n_tiles, void* stream);
/* dst[i] = bf16(sum_r f32(src[r*n + i])), r < rows; n % 8 == 0: the f32 accumulation of the bf16 gradient chunks a rank owns in the
 * data-parallel exchange (pianobart_amd/parallel.py; replaces the logits gather + gradient reduce of nn.DataParallel, pretrain.py:63-65) */
int pb_sum_rows_bf16(const void* src, void* dst, int32_t rows, int64_t n, void* stream);

/* ---- K17: gradient accumulation over micro-batches (pb_accum.hip; an addition to ABI 10) -----------
 * dst[i] = src[i] (add = 0) or dst[i] += src[i] (add = 1) for 0 <= i < n, both f32. The reference takes one optimizer step per loader
 * batch (pretrain.py:192-196); this is the `+=` of torch's .grad between backward calls for the flat gradient buffer. Called on whole
 * flat buffers and on slot ranges of them: the pointers need 4-byte alignment only (a misaligned head and tail are done with scalar
 * accesses, the body with 16-byte ones; pointers that are offset differently from a 16-byte boundary take scalar accesses throughout).
 * Nothing outside [0, n) is read or written; no atomics (bit-reproducible); n <= 0 is a no-op that returns 0. */
int pb_accum_f32(float* dst, const float* src, int64_t n, int32_t add, void* stream);

/* ---- K18: checkpoint merging (pb_merge.hip; additions to ABI 10) -----------------------------------------------------
 * Replaces model_merging_methods/merging_methods.py (average_merging, task_arithmetic, ties_merging, mask_merging) and
 * mask_weights_utils.py of the reference's tidied tree: N fine-tuned backbones and the pre-trained one, each packed into ONE flat f32
 * vector in the order of the sorted parameter names, are merged by a handful of streaming passes. All arithmetic is float32, every
 * operation rounded once in the order DESIGN.md 9 writes it (the file is compiled without contraction: an FMA would break bit parity
 * with the reference's CPU tensors). Integer counts only, no float atomics: equal inputs give equal bytes.
 *
 * pb_merge_kth_abs: *kth_out = the exact k-th smallest (1 <= k <= n) of |x[i] - base[i]| (base != NULL; the difference is rounded once)
 *   or |x[i]|, i < n, as a radix select over the magnitude's bit pattern (non-negative floats order as unsigned integers): four
 *   streaming histogram passes over 8 bits each, top down (per-workgroup LDS bins merged by 64-bit integer atomics), a one-workgroup
 *   kernel between them that picks the bin holding the k-th element and narrows the prefix. The state lives in ws
 *   (pb_merge_kth_ws_bytes() bytes, 8-byte aligned; free for reuse by the next call on the same stream); no host round trip.
 *   *flags_out |= 1 when a magnitude has an all-ones exponent (inf / NaN); the caller zeroes and reads the word. Pointers need 4-byte
 *   alignment only (segments of a flat buffer): 16-byte loads for the body, scalar head and tail; x and base offset differently from
 *   a 16-byte boundary go scalar throughout.
 * pb_merge_sign_tally: TIES pass 1. With D_m = model[m] - pre, T_m = D_m where |D_m| >= *thresh[m] (NULL: everywhere) else 0 and
 *   s = (T_0 + T_1) + ...: tally[0] += #{s > 0}, tally[1] += #{s < 0} (device int64[2], zeroed by the caller). Reads n_models, pre,
 *   model, thresh and n of the descriptor.
 * pb_merge_apply: out[i] for i < n in one fused pass: one 16-byte load per input vector and lane, one store, registers in between.
 *   Element i is element g = g0 + i of the whole flat vector; a call over a segment draws the random mask the whole-vector call draws
 *   (g0 need not be a multiple of 4). Per model m: kind NONE: W_m = model[m]. Otherwise X = model[m] - pre (format DELTA) or model[m]
 *   (format FINETUNED); X *= 0 where it is masked -- MAGNITUDE: |X| <= *thresh[m]; RANDOM: word g & 3 of
 *   philox4x32-7(g >> 2, model_base + m, 0x4D455247, 0) under the key (low, high half of seed) < drop_thresh[m] (= uint32(float32(rate) 2^32), as
 *   64 bits so that rate 1 drops everything) --; X /= rescale[m] (pass 1 for none); W_m = pre + X (DELTA) or X. Then
 *     PB_MERGE_AVERAGE   (((0 + W_0) + W_1) + ...) / float(n_models)    (torch's sum starts at +0: all -0.0 gives +0.0; so do the TIES sums)
 *     PB_MERGE_TASK      pre + lambda * ((W_0 - pre) + (W_1 - pre) + ...)
 *     PB_MERGE_TIES      T_m as for the tally (every kind must be NONE; thresh[m] is the trim threshold); sign = sgn(s), where s == 0
 *                        the sign of tally[0] - tally[1]; kept_m = T_m where its sign equals that sign, else T_m * 0;
 *                        pre + lambda * (((kept_0 + kept_1) + ...) / max(#{kept_m != 0}, 1))
 *     PB_MERGE_MASKED    W_0 (n_models = 1): the masked model itself, for callers that run TIES over masked models
 *   2 <= n_models <= PB_MERGE_MAX_MODELS otherwise. out may not alias an input. The descriptor starts zeroed. */
#define PB_MERGE_MAX_MODELS 8
#define PB_MERGE_AVERAGE 0
#define PB_MERGE_TASK 1
#define PB_MERGE_TIES 2
#define PB_MERGE_MASKED 3
#define PB_MERGE_MASK_NONE 0
#define PB_MERGE_MASK_MAGNITUDE 1
#define PB_MERGE_MASK_RANDOM 2
#define PB_MERGE_DELTA 0
#define PB_MERGE_FINETUNED 1
typedef struct pb_merge_desc {
    const float* pre; float* out;
    const float* model[PB_MERGE_MAX_MODELS];
    const float* thresh[PB_MERGE_MAX_MODELS];   /* device scalars (pb_merge_kth_abs results) */
    int64_t* tally;
    int64_t n, g0;
    uint64_t seed;
    uint64_t drop_thresh[PB_MERGE_MAX_MODELS];
    float rescale[PB_MERGE_MAX_MODELS];
    int32_t mask_kind[PB_MERGE_MAX_MODELS];
    int32_t n_models, method, format; float lambda;
    int32_t model_base, _pad;                   /* index of model[0] in the whole merge: model m draws stream model_base + m */
} pb_merge_desc;
int64_t pb_merge_desc_bytes(void);
int64_t pb_merge_kth_ws_bytes(void);
int pb_merge_kth_abs(const float* x, const float* base, int64_t n, int64_t k, float* kth_out, int32_t* flags_out, void* ws, void* stream);
int pb_merge_sign_tally(const pb_merge_desc* d, void* stream);
int pb_merge_apply(const pb_merge_desc* d, void* stream);

/* ---- K25: Fisher merging (pb_fisher.hip; additions to ABI 10) ------------------------------------------------------------
 * The reference's fisher_merging (model_merging_methods/merging_methods.py:82-264): fine-tuned weights averaged element by element,
 * each model weighted by the diagonal of its own task's empirical Fisher information. Float32, every operation rounded once in the
 * order DESIGN.md 9 writes it (the file is compiled without contraction). No float atomics: equal inputs give equal bytes. Every entry
 * checks its arguments before the first HIP call (-2, pb_last_error names the field). Pointers need 4-byte alignment only (segments of
 * a flat buffer): 16-byte accesses for the body, scalar head and tail; pointers of one call that are offset differently from a
 * 16-byte boundary go scalar throughout.
 *
 * pb_fisher_rows: per row of logits (rows, C), C >= 1, with p = softmax(logits[row]): e_out[row] = sum_c sqrt(p_c) log p_c (log p = z -
 *   logsumexp; a class whose p underflows to 0 adds 0). dlogits != NULL: dlogits[row][j] = weight[row] (sqrt(p_j) - p_j sum_c sqrt(p_c)),
 *   the gradient of e_out[row] with sqrt(p) held constant, as the reference detaches it; weight NULL = 1, weight 0 = a row of zeros.
 *   One wave per row, 4 rows per workgroup.
 * pb_fisher_accum: F[i] = F[i] + g[i] * g[i], i < n (a product and a sum, each rounded): one streaming pass per batch over the engine's
 *   flat gradient buffer.
 * pb_fisher_finish: F[i] = F[i] / float(divisor), an IEEE division (1 <= divisor <= 2^24: the examples computed); *flags |= 1 where a
 *   result is not finite (the caller zeroes and reads the word).
 * pb_fisher_norm: *norm_out = float32(sqrt(sum_i F[i]^2)), the sum in float64: per-workgroup partial sums in fixed slots of ws
 *   (pb_fisher_norm_ws_bytes() bytes, 8-byte aligned), folded by one workgroup. The order of the additions depends on n alone.
 * pb_fisher_merge: with Fp_m = fisher[m] + minimal and k_m = coef[m] * Fp_m:
 *     out[i] = (((0 + k_0 * model[0]) + k_1 * model[1]) + ...) / (((0 + k_0) + k_1) + ...)
 *   in one fused pass: one 16-byte load per input vector and lane, one store. 2 <= n_models <= PB_MERGE_MAX_MODELS; coef[m] and
 *   minimal positive and finite (then no denominator is 0); out may not alias an input. The descriptor starts zeroed. */
typedef struct pb_fisher_desc {
    float* out;
    const float* model[PB_MERGE_MAX_MODELS];
    const float* fisher[PB_MERGE_MAX_MODELS];
    int64_t n;
    float coef[PB_MERGE_MAX_MODELS];
    float minimal; int32_t n_models;
} pb_fisher_desc;
int64_t pb_fisher_desc_bytes(void);
int64_t pb_fisher_norm_ws_bytes(void);
int pb_fisher_rows(const float* logits, const float* weight, float* e_out, float* dlogits, int64_t rows, int32_t C, void* stream);
int pb_fisher_accum(float* F, const float* g, int64_t n, void* stream);
int pb_fisher_finish(float* F, int64_t n, int64_t divisor, int32_t* flags, void* stream);
int pb_fisher_norm(const float* F, int64_t n, void* ws, float* norm_out, void* stream);
int pb_fisher_merge(const pb_fisher_desc* d, void* stream);

/* ---- K26: RegMean merging (pb_regmean.hip; additions to ABI 10) ----------------------------------------------------------
 * The reference's regmean_merging (model_merging_methods/merging_methods.py:266-416): per linear layer W^T = (sum_m G_m)^-1 sum_m G_m W_m^T
 * with G_m = X_m^T X_m / rows the Gram matrix of the layer's inputs under model m. All matrices are row-major f32 with a leading dimension
 * in elements. No float atomics: equal inputs give equal bytes. Every entry checks its arguments before the first HIP call (-2,
 * pb_last_error names the field); 1 <= K <= 32768.
 *
 * pb_gram_accum: G (K, K) += X^T X for X (T, K), dtype PB_BF16 (bf16 MFMA, f32 accumulation) or PB_F32 (f32-input MFMA: an f32 fma
 *   chain), 1 <= T <= 2^30, any K, ldx, alignment of X to its element (16-byte loads where X and ldx allow them). Only the 128 x 128 tiles
 *   on and below the diagonal are computed; T is cut into chunks that go to different workgroups, each writes its partial tile to a fixed
 *   slot of ws (pb_gram_ws_bytes(T, K) bytes, 16-byte aligned; 0 for sizes the entry refuses) and the slots are folded in chunk order, in
 *   an order that depends on (T, K) alone. The new G[i][j], j <= i, is stored at (i, j) and (j, i): G comes out symmetric bit for bit
 *   whatever its upper triangle held.
 * pb_regmean_scale: out[i][j] = G[i][j] * (i == j ? diag : off), one multiplication per element (reduce_non_diagonal_elements with
 *   off = float32(ratio), diag = float32(float32(1 - ratio) + float32(ratio))). out may be G (then ldo == ldg).
 * pb_chol_factor: A (K, K) -> its lower Cholesky factor L in place, the strict upper triangle (never read) set to 0. Blocks of 64 columns:
 *   the diagonal block by one workgroup in LDS, the panel below it by forward substitution against that block, the trailing matrix
 *   through pb_gemm (PB_F32, alpha = -1, PB_GEMM_ACCUM). *info (device int32, zeroed by the caller) is set to 1 + j for the first column j
 *   whose pivot is <= 0 or not finite if it is still 0, and left alone otherwise: one word may serve several calls of one stream and is
 *   read once at the end. After such a pivot L holds inf / NaN; nothing is read or written out of bounds.
 * pb_chol_solve: R (K, nrhs) -> Z with L L^T Z = R in place: forward then backward substitution, blocked as the factor. nrhs >= 1.
 * pb_transpose_f32: dst (cols, rows) = src (rows, cols)^T, a copy (the (out, in) layout of a Linear.weight from the solve's (in, out)). */
int64_t pb_gram_ws_bytes(int64_t T, int32_t K);
int pb_gram_accum(const void* X, int64_t ldx, int32_t dtype, int64_t T, int32_t K, float* G, int64_t ldg, void* ws, void* stream);
int pb_regmean_scale(const float* G, int64_t ldg, float* out, int64_t ldo, int32_t K, float off, float diag, void* stream);
int pb_chol_factor(float* A, int64_t ld, int32_t K, int32_t* info, void* stream);
int pb_chol_solve(const float* L, int64_t ldl, int32_t K, float* R, int64_t ldr, int32_t nrhs, void* stream);
int pb_transpose_f32(const float* src, int64_t lds, float* dst, int64_t ldd, int32_t rows, int32_t cols, void* stream);

/* ---- K19: set metrics for generated pieces (pb_metrics.hip; additions to ABI 10) ----------------------------------------
 * Per-piece musical features, pairwise feature distances, their moments and a Gaussian kernel density estimate: the device half of
 * pianobart_amd.metrics. Integer counts and fixed-order floating-point sums only: equal inputs give equal bytes.
 * Every entry checks its arguments before the first HIP call (-2, pb_last_error names the field).
 *
 * pb_piece_features: feat (N, 288) int32 from ids16 (N, S, 8) int16, 16-byte aligned. The notes of piece n are its rows
 *   start[n] (0 when start is NULL) .. L - 1, L = the first row in which any head's id is >= pad8[h] (S if none). pad8: 8 HOST
 *   int32, each 1 .. 1082; pitch_of: pad8[3] device int16, the MIDI number of a pitch id or -1 (percussion); dur_pos: pad8[4]
 *   device int32, the length of a duration id in positions. The columns are the table of DESIGN.md 10. One workgroup per piece, a
 *   workgroup sweeping over several pieces when they are short or many.
 * pb_pairwise_l2: D[i, j] = sqrt(sum_f (A[i, f] - B[j, f])^2), A (N, F), B (M, F), D (N, M) f32, 1 <= F <= 144; one f32 chain over
 *   f = 0 .. F - 1 of the squared differences (never |a|^2 + |b|^2 - 2ab): equal rows give exactly 0.
 * pb_sample_moments: out[0 .. 5] = n, sum, sum of squares, 0, min, max (device doubles) of the samples of D (N, M) f32: all of it,
 *   or with upper = 1 (N == M) the strict upper triangle j > i. f64 throughout, fixed-order partials in ws.
 * pb_kde_eval: dens[g] = 1 / (n h sqrt(2 pi)) sum_s exp(-(grid[g] - s)^2 / (2 h^2)) over the same samples, 1 <= G <= 4096, n >= 1.
 *   Terms in f32 (one exp2 of (grid[g] - s)^2 * float32(-log2(e) / (2 h^2))), summed in f64: per sample slab one partial row in ws,
 *   the slabs summed front to back by a second kernel.
 * pb_metrics_ws_bytes: the bytes of ws (8-byte aligned, free for reuse by the next call on the same stream) that
 *   pb_sample_moments and pb_kde_eval need for an (N, M) matrix and G grid points. */
int64_t pb_metrics_ws_bytes(int64_t N, int64_t M, int32_t G);
int pb_piece_features(const int16_t* ids16, const int32_t* start, const int32_t* pad8, const int16_t* pitch_of, const int32_t* dur_pos,
                      int32_t* feat, int32_t N, int32_t S, void* stream);
int pb_pairwise_l2(const float* A, const float* B, float* D, int32_t N, int32_t M, int32_t F, void* stream);
int pb_sample_moments(const float* D, int64_t N, int64_t M, int32_t upper, double* out, void* ws, void* stream);
int pb_kde_eval(const float* D, int64_t N, int64_t M, int32_t upper, const float* grid, int32_t G, double h, double* dens, void* ws, void* stream);

/* ---- K20: copy detection (pb_runs.hip; additions to ABI 10) -----------------------------------------------------------------
 * The longest run of consecutive notes that a generated piece shares with a corpus piece: the device half of pianobart_amd.novelty
 * (DESIGN.md 11). Integers and integer maxima only: equal inputs give equal bytes, whatever the order of workgroups or chunks.
 * Every entry checks its arguments before the first HIP call (-2, pb_last_error names the field).
 *
 * pb_piece_keys: keys (N, S) uint32 and klen (N) int32 from ids16 (N, S, 8) int16, 16-byte aligned, 1 <= S <= 4096. The notes of a
 *   piece, start, pad8 and pitch_of are those of pb_piece_features. A piece of n notes has K = max(n - 1, 0) keys; key t - 1
 *   describes note t relative to note t - 1: bits 0..11 the pitch field (mode 0, exact: the pitch id; mode 1, interval:
 *   1088 + pitch_of[id_t] - pitch_of[id_t-1] when both are >= 0, else 2304 + the pitch id), bits 12..22 the position id, bits 23..24
 *   the bar step (0, 1, 2; 3 = anything else), bits 25..31 zero. keys[n][K ..] = 0xFFFFFFFF ("no key").
 * pb_shared_runs: A (N, Sa) with alen (N), B (M, Sb) with blen (M): key rows and their lengths (clamped to 0 .. Sa / Sb), 1 <= Sa, Sb
 *   <= 4096, min_run >= 1. A value with bit 31 set is "no key" and matches nothing. run(p, q) = A[p] == B[q] ? run(p - 1, q - 1) + 1 : 0.
 *   R[i][j] (N, M; may be NULL) = max over p, q of run(p, q); run_end[i][p] (N, Sa) = max over j, q of run(p, q) where that is
 *   >= min_run, else 0; best[i] (N, int64) = (max_j R[i][j]) << 32 | (0xFFFFFFFF - (j* + j_base)), j* the smallest j that attains the
 *   maximum, 0 when the maximum is 0. exclude_self = 1 (N == M): the pair i == j + j_base contributes nothing. accumulate = 0 clears
 *   run_end and best on the stream first; accumulate = 1 maxes into them: a corpus fed in chunks of M pieces, j_base = the chunk's
 *   first piece. R is always written whole. N = 0 or M = 0 is no error.
 * pb_runs_tile: the corpus pieces one workgroup of pb_shared_runs takes. */
int pb_runs_tile(void);
int pb_piece_keys(const int16_t* ids16, const int32_t* start, const int32_t* pad8, const int16_t* pitch_of, uint32_t* keys, int32_t* klen,
                  int32_t N, int32_t S, int32_t mode, void* stream);
int pb_shared_runs(const uint32_t* A, const int32_t* alen, int32_t N, int32_t Sa, const uint32_t* B, const int32_t* blen, int32_t M, int32_t Sb,
                   int32_t min_run, int32_t exclude_self, int32_t j_base, int32_t* R, int32_t* run_end, int64_t* best, int32_t accumulate,
                   void* stream);

/* ---- K21: copy detection that survives edits (pb_align.hip; additions to ABI 10) ---------------------------------------------------
 * Smith-Waterman local alignment with a linear gap penalty over the keys of pb_piece_keys: the device half of
 * pianobart_amd.novelty.local_alignments. Integers and integer maxima only: equal inputs give equal bytes, whatever
 * the order of lanes, waves, workgroups or chunks. The arguments are checked before the first HIP call (-2, pb_last_error names the
 * field).
 *
 * pb_local_align: A, alen, N, Sa, B, blen, M, Sb as in pb_shared_runs (lengths clamped to 0 .. Sa / Sb, 1 <= Sa, Sb <= 4096, a value
 *   with bit 31 set matches nothing, not even itself). Penalties are positive numbers: match 1 .. 8, mismatch 1 .. 16, gap 1 .. 16;
 *   min_score >= 1. For a pair, cell (p, q) holds P = H << 12 | (4095 - start), H the score of the best local alignment that ends
 *   there, start the A index of its first matched key, P = 0 "no alignment ends here":
 *     s = (A[p] == B[q]) ? +match : -mismatch
 *     d = max(P(p - 1, q - 1), 4095 - p) + (s << 12)
 *     r = max(d, P(p - 1, q) - (gap << 12), P(p, q - 1) - (gap << 12))
 *     P(p, q) = r >= 4096 ? r : 0,   P(-1, .) = P(., -1) = 0
 *   Among alignments of equal score the smallest start is kept. Only match cells (A[p] == B[q]) are recorded:
 *   score[i][j] (N, M; may be NULL) = max over match cells of H; align_end[i][p] (N, Sa) = max over j and over match cells (p, q) of
 *   P(p, q) where its H >= min_score, else 0 (H = v >> 12, start = 4095 - (v & 4095): the aligned region that ends at key p covers
 *   the keys start .. p); best[i] (N, int64) = (max_j score[i][j]) << 32 | (0xFFFFFFFF - (j* + j_base)), j* the smallest j that
 *   attains the maximum, 0 when the maximum is 0 (the packing of pb_shared_runs). exclude_self, j_base and accumulate as in
 *   pb_shared_runs: accumulate = 0 clears align_end and best on the stream first, accumulate = 1 maxes into them. score is always
 *   written whole. N = 0 or M = 0 is no error.
 * pb_align_block: the B columns one sweep of a wave covers. */
int pb_align_block(void);
int pb_local_align(const uint32_t* A, const int32_t* alen, int32_t N, int32_t Sa, const uint32_t* B, const int32_t* blen, int32_t M, int32_t Sb,
                   int32_t match, int32_t mismatch, int32_t gap, int32_t min_score, int32_t exclude_self, int32_t j_base,
                   int32_t* score, int32_t* align_end, int64_t* best, int32_t accumulate, void* stream);

/* ---- K22: repetition structure of a piece (pb_structure.hip; additions to ABI 10) ------------------------------------------------------
 * How much of a bar returns 1 .. 64 bars later: the device half of pianobart_amd.structure. Integers and integer sums
 * only: equal inputs give equal bytes, and a permutation of a piece's note rows gives the same row. The arguments are checked before
 * the first HIP call (-2, pb_last_error names the field).
 *
 * pb_piece_structure: out (N, 264) int32 from ids16 (N, S, 8) int16, 16-byte aligned, 1 <= S <= 4096. The notes of a piece, start,
 *   pad8 and pitch_of are those of pb_piece_features. A note has its bar id b (head 0), its position id p (head 1) and a pitch field
 *   f: mode 0 (exact) the pitch id (head 3); mode 1 (pitch class) pitch_of[id] % 12 where pitch_of[id] >= 0, else 12 + id. Per bar
 *   O_b = the set of p and N_b = the set of (p, f) of its notes; a bar id without a note between the smallest and the largest one
 *   is a bar with empty sets. With W = largest - smallest bar id + 1 and X = O or N, for l = 1 .. 64:
 *     I_X[l] = sum over the bar pairs (b, b + l) inside the span of |X_b ^ X_{b+l}|,   T_X[l] = sum over the same pairs of |X_b| + |X_{b+l}|
 *   (both 0 for l >= W). Columns: 0 notes, 1 W (0 without a note), 2 sum_b |O_b|, 3 sum_b |N_b|, 4 distinct bar ids, 5..7 zero,
 *   8..71 I_O[1..64], 72..135 T_O[1..64], 136..199 I_N[1..64], 200..263 T_N[1..64]. One workgroup per piece, a workgroup sweeping over
 *   several pieces when they are short or many (at most 1024 workgroups). N = 0 is no error.
 * pb_structure_lags / pb_structure_cols: 64 and 264. */
int pb_structure_lags(void);
int pb_structure_cols(void);
int pb_piece_structure(const int16_t* ids16, const int32_t* start, const int32_t* pad8, const int16_t* pitch_of,
                       int32_t* out, int32_t N, int32_t S, int32_t mode, void* stream);

/* ---- K23: harmony of a piece (pb_harmony.hip; additions to ABI 10) ----------------------------------------------------------------------
 * The pitch classes of a piece's bars: the device half of pianobart_amd.harmony. Integers and integer sums only: equal
 * inputs give equal bytes, and a permutation of a piece's note rows gives the same row. The arguments are checked before the first HIP
 * call (-2, pb_last_error names the field).
 *
 * pb_piece_harmony: out (N, 228) int64 from ids16 (N, S, 8) int16, 16-byte aligned, 1 <= S <= 4096. The notes of a piece, start, pad8
 *   and pitch_of are those of pb_piece_features; bars and W are those of pb_piece_structure. A note is pitched when
 *   pitch_of[id of head 3] >= 0, its class is c = pitch_of[id] % 12. h_b[c] = the pitched note rows of bar b with class c (a multiset),
 *   n_b their number; a window of w bars (w = 1, 4) starting at b = 0 .. W - w has the sum of its bars' histograms. table: device
 *   int64 (4097), table[k] = round(k log2(k) 2^20), table[0] = table[1] = 0; X(window) = table[n] - sum_c table[h[c]]. D_k = k + {0, 2, 4,
 *   5, 7, 9, 11} mod 12; best(h) = max_k of the sum of h over D_k, key(h) the smallest k attaining it. For l = 1 .. 64 over the bar
 *   pairs (b, b + l) inside the span: I_H[l] = sum of sum_c min(h_b[c], h_{b+l}[c]), T_H[l] = sum of n_b + n_{b+l},
 *   I_X[l] = sum of max over t = 0 .. 11 of sum_c min(h_b[c], h_{b+l}[(c + t) % 12]).
 *   Columns: 0 notes, 1 W (0 without a note), 2 pitched notes P, 3 percussion notes, 4 bars with n_b > 0, 5 K* = key(g) of the whole
 *   piece's histogram g, 6 SC = best(g), 7 zero, 8..19 g[0..11], 20..27 the window block of w = 1, 28..35 that of w = 4 (windows,
 *   non-empty windows, sum n, sum X, sum best, non-empty windows with key == K*, key changes between consecutive non-empty windows,
 *   sum of the classes present), 36..99 I_H[1..64], 100..163 T_H[1..64], 164..227 I_X[1..64]. One workgroup per piece, a workgroup
 *   sweeping over several pieces when they are short or many (at most 1024 workgroups). N = 0 is no error.
 * pb_harmony_lags / pb_harmony_cols: 64 and 228. */
int pb_harmony_lags(void);
int pb_harmony_cols(void);
int pb_piece_harmony(const int16_t* ids16, const int32_t* start, const int32_t* pad8, const int16_t* pitch_of, const int64_t* table,
                     int64_t* out, int32_t N, int32_t S, void* stream);

/* ---- K24: texture of a piece (pb_texture.hip; additions to ABI 10) ----------------------------------------------------------------------
 * How many pitches sound at once, in absolute time: the device half of pianobart_amd.texture. Integers and integer sums
 * only: equal inputs give equal bytes, and a permutation of a piece's note rows gives the same row. The arguments are checked before
 * the first HIP call (-2, pb_last_error names the field).
 *
 * pb_piece_texture: out (N, 64) int32 from ids16 (N, S, 8) int16, 16-byte aligned, 1 <= S <= 4096. The notes of a piece, start, pad8,
 *   pitch_of and dur_pos are those of pb_piece_features; bar ids, b_lo and W those of pb_piece_structure. bar_pos: device int32
 *   (pad8[6]), the positions of a bar of a time-signature id; the kernel clamps it to 1 .. 1024 and a duration to 1 .. 4096. Bar index
 *   b = bar id - b_lo; ts(b) = the time-signature id (head 6) of the note row of bar b with the smallest (position id, time-signature
 *   id), of bar b - 1 for a bar without a note; len(b) = bar_pos[ts(b)]; B(b) = the sum of len over the bars before b. A pitched note
 *   (k = pitch_of[id of head 3] >= 0) has its onset t = B(b) + position id, its length d = max(dur_pos[id of head 4], 1) and its end
 *   e = t + d. Pitch k sounds at step tau if one of its notes has t <= tau < e; c(tau) = the number of pitches that sound.
 *   Columns: 0 notes, 1 pitched notes P, 2 W; with P = 0 the others are 0. 3 T = max e - min t, 4 / 5 the steps of [min t, max e) with
 *   c >= 1 / c >= 2, 6 A = the sum of c over the steps, 7 max c, 8 D = the sum of d, 9 X = the distinct (k, t) for which a note of the
 *   same k has t' < t < e', 10 Y = P - G, 11 O = distinct t, 12 notes with e > B(b) + len(b) of their own bar, 13 notes with position
 *   id >= len(b), 14 G = distinct (k, t), 15 zero, 16..32 the steps with c = 0, 1, .., 15, >= 16 (sum T), 33..41 the onsets at which
 *   1, .., 8, >= 9 distinct k start (sum O), 42..57 the gaps g between consecutive distinct onsets by min(floor(log2 g), 15)
 *   (sum O - 1), 58..63 zero. One workgroup per piece, a workgroup sweeping over several pieces when they are short or many (at most
 *   1024 workgroups). N = 0 is no error.
 * pb_texture_cols: 64. */
int pb_texture_cols(void);
int pb_piece_texture(const int16_t* ids16, const int32_t* start, const int32_t* pad8, const int16_t* pitch_of, const int32_t* dur_pos,
                     const int32_t* bar_pos, int32_t* out, int32_t N, int32_t S, void* stream);

/* ---- K27: embedding-space set metrics (pb_embed.hip; additions to ABI 10) ------------------------------------------------------------
 * One vector per piece from the encoder's last hidden state, float64 set moments for a Frechet distance, squared distances for rows up to
 * 4096 wide and the k-nearest-neighbour counts of precision / recall / density / coverage (Naeem et al. 2020): the device half of
 * pianobart_amd.embedding. No float atomics; every floating-point sum has a fixed order; integer atomics only where the
 * result is an integer sum: equal inputs give equal bytes. Matrices are row-major with a leading dimension in elements. Every entry
 * checks its arguments before the first HIP call (-2, pb_last_error names the field).
 *
 * pb_pool_rows: out[b, c] = (sum over s with mask[b, s] != 0 of H[(b S + s) ldh + c]) / count_b as f32 and count[b] = the number of such s
 *   as int32, for H bf16 or f32 (dtype PB_BF16 / PB_F32), 1 <= B <= 65535, 1 <= S <= 65536, d >= 1, ldh >= d. mask (B, S) f32 or NULL = every row;
 *   out (B, d) f32 with ldo >= d. The sum over s runs in f64: S is cut into 16 slices of ceil(S / 16) rows, each summed front to back,
 *   the slices added in order; one division in f64, one rounding to f32. count_b = 0 gives a zero row. 16-byte loads where H and ldh
 *   allow them, element loads otherwise.
 * pb_embed_moments: mean (d) f64 = sum_n X[n] / N and C (d, d) f64 with ldc >= d, C[i][j] = sum_n (X[n][i] - mean[i]) (X[n][j] - mean[j]),
 *   for X (N, d) f32 with ldx >= d, 2 <= N <= 2^24, 1 <= d <= 4096. Two passes over X; N is cut into at most 16 chunks of a multiple of
 *   16 rows that depend on N alone, each chunk writes its partial column sums and its partial 64 x 64 tiles to fixed slots of ws
 *   (pb_embed_ws_bytes(N, d) bytes, 8-byte aligned; 0 for sizes the entry refuses) and the slots are folded in chunk order. Only the
 *   tiles on and below the diagonal are computed; C[i][j], j <= i, is stored at (i, j) and (j, i): C is symmetric bit for bit. Plain f64
 *   fma. The caller divides by N - 1.
 * pb_sqdist: D2[i ldd + j] = sum_f (A[i lda + f] - B[j ldb + f])^2 for A (N, d), B (M, d) f32, 1 <= d <= 4096, 1 <= N, M <= 2^20: one f32 fma
 *   chain over f = 0 .. d - 1 per element (never |a|^2 + |b|^2 - 2ab), so equal rows give exactly 0 and the value depends on no tiling.
 *   64 x 64 tile per workgroup, 4 x 4 per thread, slabs of 32 features staged through LDS (16-byte loads where A / B and lda / ldb allow
 *   them). A and B may be the same buffer; D2 must not overlap them.
 * pb_knn_radius: rad[i] = the k-th smallest of D2[i ldd + j] over 0 <= j < N, j != r0 + i, for the rows r0 .. r0 + n - 1 of a set's own
 *   (N, N) matrix passed as the (n, N) block D2; 1 <= n, r0 >= 0, r0 + n <= N <= 2^24, 1 <= k <= min(N - 1, 64). A radix selection on the
 *   bits: the result is a value of the input.
 * pb_ball_counts: over D2 (n, M) with ldd, rad_ref (M), rad_gen (n): row_hits[i] += #{j : D2[i][j] < rad_ref[j]}, col_hits[j] += #{i :
 *   D2[i][j] < rad_ref[j]}, col_hits_gen[j] += #{i : D2[i][j] < rad_gen[i]} (int32, zeroed by the caller; strict <). Integer atomics:
 *   feeding the rows in blocks gives the one-shot counts. 1 <= n <= 2^20, 1 <= M <= 2^24. */
int64_t pb_embed_ws_bytes(int64_t N, int32_t d);
int pb_pool_rows(const void* H, int64_t ldh, int32_t dtype, const float* mask, float* out, int64_t ldo, int32_t* count, int32_t B, int32_t S,
                 int32_t d, void* stream);
int pb_embed_moments(const float* X, int64_t ldx, int64_t N, int32_t d, double* mean, double* C, int64_t ldc, void* ws, void* stream);
int pb_sqdist(const float* A, int64_t lda, const float* B, int64_t ldb, float* D2, int64_t ldd, int32_t N, int32_t M, int32_t d, void* stream);
int pb_knn_radius(const float* D2, int64_t ldd, int32_t n, int32_t N, int32_t r0, int32_t k, float* rad, void* stream);
int pb_ball_counts(const float* D2, int64_t ldd, int32_t n, int32_t M, const float* rad_ref, const float* rad_gen, int32_t* row_hits,
                   int32_t* col_hits, int32_t* col_hits_gen, void* stream);

/* ---- device-side corruption for the pre-train step (distributional counterpart of gen_mask's
 * TokenMask n=0 branch, pretrain.py:276-295) and decoder shift-right (pretrain.py:132-139) ---------*/
int pb_shift_right(const int16_t* ids, const int16_t* sos_row /*device 8*/, int16_t* out, int32_t B, int32_t S, void* stream);
/* Replaces Pretrainer.gen_mask (pretrain.py:211-546): one workgroup corrupts one (S,8) sequence in LDS.
 * choice (B) int32 device, 1..5 (other values / NULL: drawn uniformly in-kernel, reported in choice_out if given);
 * out (B,S,8) int16, loss_mask (B,S,8) f32 (per-position mask repeated over the 8 columns, pretrain.py:141-142).
 * pad_row / mask_row / n_tokens: HOST arrays of 8. mask_percent is a double: int(l * p) and round(l * p) must come out as in
 * Python. Same distributions as the reference, Philox instead of MT19937. */
int pb_corrupt(const int16_t* ids, int16_t* out, float* loss_mask, const int32_t* choice, int32_t* choice_out, int32_t B,
               int32_t S, double mask_percent, uint64_t seed, const int16_t* pad_row, const int16_t* mask_row,
               const int32_t* n_tokens, void* stream);
/* The same kernel with its random DECISIONS supplied by the caller instead of drawn from Philox: what is left is the deterministic
 * part of gen_mask, which must reproduce the reference's outputs bit for bit when fed the reference's own decisions
 * (tests/test_corrupt_gpu.py, tests/golden/g6_gen_mask.npz). choice (B) int32 device, required. decisions: (B, dec_stride) int32
 * device, dec_stride >= pb_corrupt_replay_stride(S); per sample, by choice:
 *   1 TokenDeletion        dec[i] != 0: position i is deleted (the shuffled maskpos of pretrain.py:221-226); i < S
 *   2 TokenMask            dec[i] = 0 untouched, 1 in mask80 (MASK row), 2 in rand10 (row i of rand_rows), 3 in cur10; i < S
 *   3 SentencePermutation  dec[bar] = place of bar value `bar` in the shuffled bar order (pretrain.py:385-386)
 *   4 TokenInfilling       dec[attempt * S + step] = -1 (random.random() >= p/3: copy the row) or the np.random.poisson(3) draw of a
 *                          span that starts at this step; attempt < 10, steps in the order the reference's while loop takes them
 *   5 DocumentRotation     dec[0] = the rotation offset (random.randint(0, l-1))
 * rand_rows: (B,S,8) int16 device, the get_rand_tok() rows of choice 2 (may be NULL when no decision is 2). */
int pb_corrupt_replay(const int16_t* ids, int16_t* out, float* loss_mask, const int32_t* choice, int32_t B, int32_t S,
                      double mask_percent, const int32_t* decisions, int64_t dec_stride, const int16_t* rand_rows,
                      const int16_t* pad_row, const int16_t* mask_row, void* stream);
int64_t pb_corrupt_replay_stride(int32_t S);
/* Whole-piece augmentation in front of the corruption: piece b of ids (B,S,8) int16 is shifted along three axes, a = 0
 * pitch (head 3), 1 velocity (head 5), 2 tempo (head 7), by one amount per axis; the other five heads are copied. Per axis:
 *   coord (3, 1088) int16 device: coord[a][id] = the id's coordinate >= 0, or -1 = never touched (specials, percussion pitches)
 *   id_at (3, 1088) int16 device: id_at[a][c] = the id of coordinate c, 0 <= c < ncoord (total: the inverse of coord)
 *   plan  (3, 6) int32 HOST: lo, hi, blo, bhi, ncoord, thresh -- the request lo <= 0 <= hi, the coordinate bounds 0 <= blo <= bhi < ncoord
 *         <= 1088, thresh = the apply threshold as uint32 bits (0xFFFFFFFF: always)
 * Piece b, axis a: cmin, cmax = the extremes of coord[a][ids[b, i, head]] over the positions with a coordinate (none: s = 0); flo =
 * max(lo, blo - cmin), fhi = min(hi, bhi - cmax); flo > 0 or fhi < 0 (the piece lies outside the bounds, or fills them): s = 0; else r =
 * philox4x32(0, b, a, 0xA06) under the key (seed low, high), s = flo + ((uint64)r.x * (fhi - flo + 1) >> 32), and s = 0 if thresh !=
 * 0xFFFFFFFF and r.y >= thresh. shifts[b * 3 + a] = s (int32 device); out = id_at[a][coord + s] where the id has a coordinate, else the id.
 * So no note is clipped or wrapped. out == ids (in place) is allowed, a partial overlap is refused; 1 <= B <= 65535, 1 <= S <= 65536; ids,
 * out and the tables 16-byte aligned. Equal inputs and seed give equal bytes. tests/augment_ref.py restates it. */
int pb_augment(const int16_t* ids, int16_t* out, int32_t* shifts, int32_t B, int32_t S, const int16_t* coord, const int16_t* id_at,
               const int32_t* plan, uint64_t seed, void* stream);

/* ---- K14: fine-tune heads, exact f32 (model.py:128-143 SelfAttention, :165-218 SequenceClassification, :220-232 Excitation,
 * :236-272 TokenClassification; loss finetune.py:121-129). Their matrix products are pb_gemm (f32) calls.
 * pb_eltwise_fwd: y = dropout(act(x)), op 1 tanh / 2 relu / 3 sigmoid / 4 identity / 5 x * x2; n elements;
 *   dropout by the step's Philox stream (seed, site), p_drop = 0 disables it.
 * pb_eltwise_bwd: dx = dy * mask * act'(.) with the derivative taken from the PRE-dropout output `y` (op 5: y = x, also dx2).
 * pb_softmax_dim1_*: F.softmax(x, dim=1) of x (B, S, R) and its backward (model.py:140).
 * pb_ce_rows: loss[row] = CrossEntropy(logits[row, :C], target[row]) (reduction='none'), argmax[row] (first maximum, may be
 *   NULL) and, if dlogits != NULL, dlogits = (softmax - onehot) * coef[0] * weight[row] (weight / coef may be NULL = 1).
 *   A target outside [0, C) (nn.CrossEntropyLoss's ignore_index = -100) gives loss 0 and an all-zero dlogits row; argmax is written. */
int pb_eltwise_fwd(int32_t op, const float* x, const float* x2, float* y, int64_t n, uint64_t seed, uint32_t site, float p_drop, void* stream);
int pb_eltwise_bwd(int32_t op, const float* y, const float* x2, const float* dy, float* dx, float* dx2, int64_t n, uint64_t seed,
                   uint32_t site, float p_drop, void* stream);
int pb_softmax_dim1_fwd(const float* x, float* y, int32_t B, int32_t S, int32_t R, void* stream);
int pb_softmax_dim1_bwd(const float* y, const float* dy, float* dx, int32_t B, int32_t S, int32_t R, void* stream);
int pb_ce_rows(const float* logits, const int32_t* target, const float* weight, const float* coef, float* loss, float* dlogits,
               int32_t* argmax, int64_t rows, int32_t C, void* stream);
/* Decoder label-embedding swap of the velocity task (PianoBart.change_decoder_embedding, PianoBart.py:88-91; model.py:242-245):
 * pb_gather_rows: out[t] = table[ids[t]] + bias for a small projected label table (nrows x d, f32); pb_gather_rows_bwd: dtable[r] =
 * sum of dout[t] over ids[t] == r (sequential per element: deterministic). pb_dropout: y = x * mask / (1 - p) in storage dtype
 * (BART drops after layernorm_embedding); the same call on the gradient is its backward. */
int pb_gather_rows(const float* table, const int32_t* ids, const float* bias, float* out, int64_t T, int32_t d, int32_t nrows, void* stream);
int pb_gather_rows_bwd(const float* dout, const int32_t* ids, float* dtable, int64_t T, int32_t d, int32_t nrows, void* stream);
int pb_dropout(const void* x, void* y, int64_t n, int32_t dtype, uint64_t seed, uint32_t site, float p_drop, void* stream);
/* The optional regulariser of the fine-tune loop, `loss += weight * torch.norm(param, p=2)` for every parameter tensor
 * (finetune.py:241-243): *loss_acc += weight * ||p||_2 (if loss_acc != NULL) and g += weight * p / ||p||_2 (if g != NULL; 0 where the
 * norm is 0, as torch's norm backward). p, g: n f32 elements, any alignment; scratch: pb_l2_penalty_scratch_floats() floats. */
int pb_l2_penalty(const float* p, float* g, int64_t n, float weight, float* scratch, float* loss_acc, void* stream);
int64_t pb_l2_penalty_scratch_floats(void);

/* ---- K13: batch-1 KV-cached decode (model.py:28-66) --------------------------------------------------------------
 * pb_gemv: y[n] = act(sum_k W[n][k] x[k] + bias[n]), W (N,K) row-major in dtype, x (K) dtype, y dtype or f32, gelu = exact erf GELU.
 * pb_attn_decode: one query (H*hd) against cached K/V rows (element (j,h,c) at ptr[j*ss + h*hd + c]), keys 0..Sk-1, optional
 * key mask (Sk) float; a row with no visible key gives zeros. head_dim 32, 64, 96 or 128, Sk <= 8192.
 * pb_decode_step: one decoder token through all layers: embed(tok16) + pos[i] -> ND x [self-attn with K/V appended at row i,
 * cross-attn on the cached encoder K/V, FFN] -> logits (vocab) f32. All pointers device pointers, weights in dtype storage,
 * biases / LayerNorm / tables f32. */
int pb_gemv(const void* W, const void* x, const float* bias, void* y, int32_t N, int32_t K, int32_t dtype, int32_t y_f32, int32_t gelu, void* stream);
int pb_attn_decode(const void* q, const void* k_cache, const void* v_cache, void* out, const float* key_mask, int32_t H, int32_t Sk,
                   int32_t hd, int64_t k_ss, int64_t v_ss, float scale, int32_t dtype, void* stream);
#define PB_DECODE_MAX_LAYERS 48
#define PB_DECODE_MAX_SPLITS 16
typedef struct pb_decode_layer {
    const void* wqkv; const float* bqkv; const void* wo; const float* bo; const float* ln1_w; const float* ln1_b;
    const void* wq_c; const float* bq_c; const void* wo_c; const float* bo_c; const float* lnc_w; const float* lnc_b;
    const void* w1; const float* b1; const void* w2; const float* b2; const float* ln2_w; const float* ln2_b;
    void* kv_self;            /* (S, 2d) dtype: k | v rows of the tokens decoded so far */
    const void* kv_cross;     /* (S_enc, 2d) dtype: encoder keys | values of this layer */
} pb_decode_layer;
typedef struct pb_decode_plan {
    int32_t dtype, d, H, ffn, S, S_enc, n_layers, vocab;
    int32_t tab_off[9]; int32_t _pad;
    const int16_t* tok16;     /* (8) current decoder input token */
    const float* ptab; const float* lin_b; const float* pos; const float* lne_w; const float* lne_b; const float* enc_mask;
    void* x; void* y1; void* yc; void* y2; void* q; void* ctx; void* a; void* g;   /* scratch rows: d (g: ffn) elements of dtype */
    float* stat;              /* 8 floats */
    float* attn_part;         /* H * PB_DECODE_MAX_SPLITS * (d / H + 4) floats, 16-byte aligned: per-(head, key split) {max, sum, output} of the single-query
                                 attention, merged by the out-projection GEMV; NULL = one workgroup per head writing ctx (the round-1 form) */
    float* logits;            /* (vocab) f32 */
    const void* head_w; const float* head_b;
    pb_decode_layer layers[PB_DECODE_MAX_LAYERS];
} pb_decode_plan;
int pb_decode_step(const pb_decode_plan* plan, int32_t i, void* stream);

/* Host-side nucleus sampling of one position (model.py:84-98 for the 8 heads): probs (heads, width) f32 softmax rows of lengths n[h],
 * thresholds p[h], u[h] = the uniform draw np.random.choice would consume. out[h] = sampled id; bit h of *tie_mask set (out[h] = -1)
 * when the result would depend on numpy's order of equal probabilities: the caller runs its numpy code for that head. No device work. */
int pb_nucleus_rows(const float* probs, int32_t width, const int32_t* n, const float* p, const double* u, int32_t heads, int32_t* out,
                    int32_t* tie_mask);
/* The fused decoder (round 3, rows and one decoder for every B in ABI 9): one step of 1 <= B <= PB_DECODE_BATCH_MAX prompts = ONE hipGraph
 * replay, for the shapes it covers (bf16, head_dim 64 / 128, d a multiple of 256 up to 1024; anything else keeps pb_decode_step or the
 * per-prompt loop). The positions live in device memory, so the launches of a step (embed, per layer {self-attention with the q|k|v
 * projections and the pending post-LN fused in, out-projection, cross-attention with its q projection, out-projection, fc1 + GELU, fc2},
 * LM heads: 6 n_layers + 2, + 1 with the device sampler) carry no position-dependent argument, and each weight byte of a step is read once
 * for all rows. B == 1 runs the single-row kernels (every load up front, no per-row flags); B > 1 their row forms, whose per-row
 * arithmetic is the same source, so a row's logits do not depend on B (tests/test_generate_batch_gpu.py). Per row in device memory: the
 * position, a done flag (B > 1: set by the sampler on a special id, by the embedding kernel at the position limit, or by the host), the
 * uniform draws.
 * pb_decode_batch.plan holds the shapes and weights as for pb_decode_step, with B-row scratch: x, y1, yc, y2, a (B, d), g (B, ffn),
 * logits (B, vocab) f32, attn_part (B, H, PB_DECODE_MAX_SPLITS, hd + 4) f32, enc_mask (B, S) f32 or NULL, tok16 unused, and
 * layers[l].kv_self / kv_cross (B, S, 2d). s_enc[b] = row b's visible encoder extent (its cross-attention split geometry).
 *   pb_batch_decoder_create     0 = created (*dec), 1 = shape not covered (return 1 is not an error), < 0 = error. The plan is copied;
 *                               its buffers (weights, K/V caches, scratch rows, attn_part) must stay alive until pb_batch_decoder_destroy.
 *   pb_batch_decoder_reset      every row at position -1 and live, ordered behind everything enqueued on `caller_stream` so far (encoder
 *                               passes, cross K/V projections); use_graph = 0 issues every step's launches directly (A/B, debugging).
 *   pb_batch_decoder_step       B == 1, host-sampled: tok8 (8 ids, host) in, the (vocab) f32 logits row of its position out (host);
 *                               returns when it landed (the token ids go up and the logits row comes down through copy nodes of the graph).
 *   pb_batch_decoder_launches   kernels per step; pb_batch_decoder_graph 1 when steps are graph replays.
 * Device-sampled decode (round 6): the per-token host round trip of model.py:42-65 (logits row down, sampling(), token up) leaves the
 * critical path. np.random.choice's uniform draws do not depend on the logits (model.py:97), so the host draws each row's (S, 8) ahead and
 * uploads them once; a one-workgroup-per-row kernel behind the LM-head GEMV then does model.py:68-107 for the 8 heads (y = logit / T,
 * softmax, nucleus with the threshold p and the draw of that position: pb_nucleus_rows' arithmetic order) and writes the next decoder
 * input on the device, so steps are enqueued back to back, 8 per hipGraph replay. The kernel also writes the raw logits row and its 8 ids
 * to pinned host logs indexed by row and position: the HOST stays the authority -- it replays each position from the logged row through
 * the reference code path (CPU softmax + nucleus, consuming the row's RNG stream exactly as the per-token loop) and, on the rare position
 * where the device's softmax rounding made another choice, rewinds that row (pb_batch_decoder_seek) and continues from its own token.
 * Results are therefore bit-identical to the per-token loop (tests/test_model_gpu.py) whatever the device sampled.
 *   pb_batch_decoder_sampler_init   temperatures, thresholds, class counts and logits offsets of the 8 heads, pad8 = the ids from which a
 *                                   sampled id is special, u = (B, S, 8) f64 draws (copied), limit = positions per row (<= S);
 *                                   fault_row / fault_period > 0 corrupt head 0's id of that row at every fault_period-th position
 *                                   (tests of the rewind path only; B == 1: row 0).
 *   pb_batch_decoder_launch         enqueue ntok steps (first_tok, (B, 8) host ids or NULL, is copied up as the rows' decoder inputs);
 *                                   ticket >= 0 for pb_batch_decoder_wait, or < 0. B > 1: a row stops by itself at the limit; B == 1:
 *                                   the steps must stay within it.
 *   pb_batch_decoder_wait           block until that run's steps are decoded and logged.
 *   pb_batch_decoder_logs           pinned logs: (B, S, vocab) f32 logits rows, (B, S, 8) int16 device-sampled ids.
 *   pb_batch_decoder_seek           tok8 != NULL: drain, then row's last decoded position = pos, its next input = tok8, live again (the
 *                                   other rows are untouched); tok8 == NULL: the row is done from the next enqueued step on (no drain).
 *   pb_batch_decoder_start          primed generation, after reset (and sampler_init): row b's last decoded position = last_pos[b]
 *                                   (-1 .. S - 1; its self-attention cache rows 0 .. last_pos[b] filled by the caller), its next input =
 *                                   next_tok[b] ((B, 8) host ids), the position it stops before = limit[b] ((B) or NULL = the sampler's
 *                                   limit, S without one); every row live. One upload for all rows; B == 1: the steps the host may
 *                                   enqueue follow (last_pos[0] + 1 .. limit[0]).
 * Samples of one prompt (several rows continuing the same piece) share its encoder pass and its cross K|V:
 *   pb_batch_decoder_share_cross    after pb_batch_decoder_create, before the first reset or launch: layers[l].kv_cross is read as
 *                                   (n_groups, S, 2d), 1 <= n_groups <= B, and row b attends to slice kv_row[b] ((B) host ints in
 *                                   [0, n_groups), every slice named by at least one row). Rows of one slice are rows of ONE prompt: their
 *                                   s_enc must be equal and so must their enc_mask rows (the grouped kernel reads a slice's mask through one
 *                                   of its rows). Everything else stays per row: kv_self, enc_mask (B, S), scratch rows, split records,
 *                                   positions, limits, done flags, draws. A bad map, or a call after a step was issued or captured, is
 *                                   refused (< 0, pb_last_error) and changes nothing. Without the call kv_cross is (B, S, 2d) and row b
 *                                   reads slice b. Where rows share a slice the cross-attention launch becomes its grouped form: one
 *                                   workgroup per (head, key split, tile of <= 4 rows of a slice) loads the K / V chunks, W_q rows and b_q
 *                                   once for the tile; each row's arithmetic, hence its logits, is bit for bit the per-row kernel's, and the
 *                                   launches per step do not change. PB_DECODE_CROSS_GROUPED=0 keeps the per-row kernel reading through
 *                                   kv_row, PB_DECODE_GROUP_TILE=2|4|8 sets the tile (developer A/B switches).
 * Forced tokens (an addition to ABI 10): part of a piece is given, per position and head, and the rest is sampled.
 *   pb_batch_decoder_force          after pb_batch_decoder_sampler_init, before the first pb_batch_decoder_start / launch of the run:
 *                                   forced = (B, S, 8) host int16 in model column order, -1 = the head is free, v >= 0 = head h of
 *                                   position i of row b is v (any id of the head's table, specials included). The table is copied to
 *                                   device memory the decoder owns. The sampler kernel then reads its position's 8 entries with its draws:
 *                                   a given head's id replaces the sampled one (in front of the done test, so a given special id stops
 *                                   the row and a given ordinary id keeps it going), a free head's id is what the unforced kernel picks
 *                                   for the same logits and draw, and a position with all 8 heads given writes its ids without sampling
 *                                   (and without logging its logits row). Launches per step and the single-stream graph do not change;
 *                                   a decoder without the call runs the unforced kernel. A value that is neither -1 nor inside its
 *                                   head's table (n8 of sampler_init), a call before sampler_init, or a call after a step was issued or
 *                                   captured is refused (< 0, pb_last_error) and changes nothing.
 * Refill (an addition to ABI 10): one decoder serves more prompts than it has rows. A row is a SLOT: when its prompt stops, the host hands
 * the slot to the next waiting prompt while the other rows decode on. The cross K|V of a prompt lives in a SLICE of kv_cross, prepared
 * ahead of the hand-over on the caller's stream.
 *   pb_batch_decoder_dynamic        after pb_batch_decoder_create, before the first step is issued or captured: layers[l].kv_cross is
 *                                   read as (n_slices, S, 2d), B <= n_slices <= 2 PB_DECODE_BATCH_MAX. Each row's visible key count, keys
 *                                   per split and slice index then live in device memory beside its position, done flag and limit
 *                                   (initially s_enc[b] of the plan and slice b; reset restores that), and the cross-attention launch is a
 *                                   third argument form of the per-row kernel that reads them there -- same arithmetic, lane-to-key mapping
 *                                   and reduction order, so a row's logits are bit for bit those of a decoder without the call. Its LDS is
 *                                   sized for the largest keys-per-split any s_enc <= S gives. The launches per step and the single-stream
 *                                   graph do not change; a decoder without the call captures exactly the kernels and arguments it captured
 *                                   before. Refused (< 0, pb_last_error, nothing changed): after a step was issued or captured, on a B = 1
 *                                   decoder, after pb_batch_decoder_share_cross (which in turn is refused on a dynamic decoder: the grouped
 *                                   kernel is not used), n_slices out of range, a second call.
 *   pb_batch_decoder_admit          puts a prompt into slot `row` of a dynamic decoder, after pb_batch_decoder_sampler_init. The row must
 *                                   have been ended by the host (pb_batch_decoder_seek with tok8 = NULL); a live row is refused. The call
 *                                   orders itself behind the work enqueued on `caller_stream` so far (an event, as reset does): the prompt's
 *                                   encoder pass, its wkv_c projections into cross slice `slice`, and its prefill into the row's kv_self rows
 *                                   0 .. last_pos. Then, in decoder-stream order, it replaces the row's key count s_enc, keys per split (the
 *                                   rule of pb_batch_decoder_create), slice, last decoded position last_pos (-1 = none), next input
 *                                   next_tok8 (8 host ids), limit and done = 0, and copies in u_row ((S, 8) f64 draws), forced_row ((S, 8)
 *                                   int16, -1 = free; NULL = every head free) and mask_row ((S) f32 into row `row` of enc_mask; NULL exactly
 *                                   when the plan has no mask). The host arrays are free when the call returns. It does not drain: no
 *                                   synchronize and no host wait; steps already enqueued for the previous occupant finish first, and the
 *                                   other rows' positions, inputs, logs, draws and flags are untouched. The logs stay indexed by row, so
 *                                   the caller reads the previous occupant's log rows before it admits. If any prompt of a run has given
 *                                   heads, the caller installs a force table up front (pb_batch_decoder_force; all -1 will do) so that the
 *                                   graphs end in the forced sampler for the whole run: a forced_row on a decoder without a table is
 *                                   refused. Checked on the host before anything changes (< 0, pb_last_error): row, slice (also: no live row
 *                                   reads it), 0 < s_enc <= S, -1 <= last_pos < limit <= S, the input ids and the forced ids against n8 of
 *                                   sampler_init, the mask rule, and more than 2 PB_DECODE_BATCH_MAX admissions in flight. Launches per
 *                                   step do not change.
 *   pb_batch_decoder_fence          `caller_stream` waits (an event, no host wait) for everything enqueued on the decoder's stream so
 *                                   far. The caller serialises its use of a cross slice and of a row's kv_self rows with it: after the
 *                                   slice's last reader was ended (seek with NULL), fence, then enqueue the next prompt's projections into
 *                                   the slice. pb_event_* / pb_stream_wait_event do not suffice here, because the decoder's stream is not
 *                                   the caller's to record on.
 * Stop at a bar (an addition to ABI 10): a row also ends at the first token whose bar id (head 0) reaches a given bar.
 *   pb_batch_decoder_stop           after pb_batch_decoder_sampler_init, before the first pb_batch_decoder_start / launch of the run:
 *                                   stop_bar = (B) host ints, 0 <= stop_bar[b] <= pad8[0] of sampler_init; pad8[0] = no stop (what
 *                                   sampler_init sets for every row). The values are stored beside the rows' positions, limits and done
 *                                   flags, in decoder-stream order (a small kernel that takes them by kernarg: the caller's array is free
 *                                   when the call returns), and pb_batch_decoder_start keeps them. The row-form sampler kernel then tests
 *                                   head 0 of the token it wrote -- after forcing, as the special-id test does -- against stop_bar[b] in
 *                                   place of pad8[0]; since stop_bar[b] <= pad8[0] the one comparison covers both rules. Heads 1 .. 7 are
 *                                   tested against pad8 as before. What a free head samples does not change, and the done flag stays a
 *                                   prediction the host confirms or rewinds. Same kernel, same kernarg layout, same launches per step: one
 *                                   more 4-byte load next to done[b] and pos[b]. A B = 1 decoder accepts the call and does nothing on the
 *                                   device (the single-row kernels have no done flag: the host ends the run). A value outside
 *                                   0 .. pad8[0], a call before sampler_init, or a call after a step was issued or captured is refused
 *                                   (< 0, pb_last_error) and changes nothing.
 *   pb_batch_decoder_admit_stop     refill: stages the stop bar (0 .. pad8[0]) that the next pb_batch_decoder_admit of `row` stores, in
 *                                   the same small kernel as the row's position, limit and done = 0. An admit without a staged value
 *                                   stores pad8[0]: a slot never inherits its previous occupant's stop. pb_batch_decoder_seek does not
 *                                   touch the value (a rewound row keeps its occupant's). Host state only, no device work. Refused (< 0,
 *                                   pb_last_error, nothing changed): not a dynamic decoder, before sampler_init, row outside 0 .. B - 1,
 *                                   a value outside 0 .. pad8[0].
 * Time-ordered sampling (an addition to ABI 10): a row whose sampled (bar, position) never goes back. With prev = the row's decoder
 * input of the position (the SOS row, the prime's last row, else the previous token after forcing) and floor[b] >= 0:
 *   head 0: the classes c < max(floor[b], prev[0] if prev[0] < pad8[0] else 0) get the quotient -inf in front of the softmax
 *           (probability exactly 0); every class from there on, the special ids included, stays free;
 *   head 1: with b0 = head 0's id after forcing, the classes c < prev[1] get -inf if prev[0] < pad8[0], prev[1] < pad8[1] and
 *           b0 == prev[0]; otherwise head 1 is sampled as ever. Heads 2 .. 7, the given heads and the draws are untouched.
 *   pb_batch_decoder_order          after pb_batch_decoder_sampler_init, before the first step of the run (pb_batch_decoder_force's window):
 *                                   floor = (B) host ints, -1 <= floor[b] < pad8[0]; -1 = the row is sampled as ever (what sampler_init sets
 *                                   for every row). Stored beside the rows' stop bars in decoder-stream order (a small kernel that takes
 *                                   them by kernarg: the caller's array is free when the call returns); pb_batch_decoder_start keeps them.
 *                                   Both sampler forms read the row's value with its position (B = 1 included: that run samples on the
 *                                   device too) and take prev from the row's decoder input on the device, which pb_batch_decoder_start /
 *                                   _seek / _admit and the sampler itself keep current. Same kernels, same kernarg layouts, same launches
 *                                   per step; the result stays a prediction the host confirms or rewinds. A value outside -1 .. pad8[0] - 1,
 *                                   a call before sampler_init, or a call after a step was issued or captured is refused (< 0,
 *                                   pb_last_error) and changes nothing.
 *   pb_batch_decoder_admit_order    refill: stages the floor (-1 .. pad8[0] - 1) that the next pb_batch_decoder_admit of `row` stores, in the
 *                                   same small kernel as the row's position, limit, stop bar and done = 0. An admit without a staged value
 *                                   stores -1: a slot never inherits its previous occupant's floor. pb_batch_decoder_seek does not touch
 *                                   the value. Host state only, no device work. Refused (< 0, pb_last_error, nothing changed): not a
 *                                   dynamic decoder, before sampler_init, row outside 0 .. B - 1, a value outside -1 .. pad8[0] - 1.
 * Vocabulary layout (an addition to ABI 10): nothing about the dictionary is compiled in. plan.vocab / plan.tab_off and sampler_init's
 * n8 / off8 / pad8 describe it; a head has 1 .. 1088 (64 x 17) classes. sampler_init picks one of two sampler forms from n8 and p8:
 * narrow while every head has <= 272 classes AND the heads with p < 1 hold at most 512 classes together (5 classes per lane, static
 * LDS, one thread per ranked class), else wide (17 classes per lane, ~104 KB of dynamic LDS, the rank counting in rounds of 512
 * threads): every dictionary inside the head limit is served. Both run the same steps in the same order,
 * take the same kernargs and honour forced ids, stop bars and bar floors alike.
 *   pb_batch_decoder_sampler_form   0 = the narrow sampler (also before sampler_init), 1 = the wide one.
 * Allowed classes (an addition to ABI 10): a row may carry an allow mask, one bit per vocabulary column (bit c & 31 of word c >> 5 =
 * column c of plan.vocab, model order). A class whose bit is 0 gets the quotient -inf in front of the softmax of its head (probability
 * exactly 0: never a nucleus candidate, never the arg-max of a p = 1 head); the draws, the temperatures, the nucleus rule, the given
 * heads, the stop test and the logged (raw) logits are untouched. A row that is time-ordered too loses the classes either rule removes,
 * and head 1's second pass keeps the allow mask. The caller keeps every head's special ids set, so a row can always end.
 *   pb_batch_decoder_allow          after pb_batch_decoder_sampler_init, before the first step of the run (pb_batch_decoder_order's window):
 *                                   masks = (n_masks, words) host words, words = ceil(plan.vocab / 32); row_mask = (B) host ints, the
 *                                   index of row b's mask, -1 = every class allowed (what sampler_init sets for every row). The table is
 *                                   copied to device memory the decoder owns (the caller's arrays are free when the call returns) and
 *                                   the indices are stored beside the rows' bar floors in decoder-stream order; pb_batch_decoder_start
 *                                   keeps them. Both sampler forms and both widths read the row's index with its position (B = 1
 *                                   included). Same kernels, same kernarg layouts, same launches per step. Refused (< 0, pb_last_error,
 *                                   nothing changed): before sampler_init, after a step was issued or captured, n_masks < 1, words !=
 *                                   ceil(vocab / 32), an index outside -1 .. n_masks - 1. A later sampler_init frees every row again.
 *   pb_batch_decoder_admit_allow    refill: stages the mask index (-1 .. n_masks - 1 of the table pb_batch_decoder_allow uploaded, which
 *                                   therefore holds the masks of ALL rows of the call from the start) that the next
 *                                   pb_batch_decoder_admit of `row` stores, in the same small kernel as the row's position, limit, stop
 *                                   bar, bar floor and done = 0. An admit without a staged value stores -1: a slot never inherits its
 *                                   previous occupant's mask. Host state only, no device work. Refused (< 0, pb_last_error, nothing
 *                                   changed): not a dynamic decoder, before sampler_init, row outside 0 .. B - 1, an index outside the table.
 * Bar schedules (an addition to ABI 10): a row may carry a bar schedule, one entry per ordinary bar id k = 0 .. pad[0] - 1: the index (in
 * pb_batch_decoder_allow's table) of the mask that heads 1 .. 7 take in a token whose bar -- head 0's id after forcing -- is k, or -1 = the
 * row's own mask. Head 0 is sampled as without a schedule (the row's own mask and bar floor); a token whose bar is special ends the row and is
 * never written: the device leaves its heads 1 .. 7 under the mask it sampled them with first (the sampler starts heads 1 .. 7 from
 * the entry of the decoder input's bar and samples them a second time only where the token's own bar names another mask). The caller stores in an entry the mask it wants IN FORCE (already intersected with the
 * row's own mask, special ids set). Draws, temperatures, nucleus rule, given heads, stop test and logged logits are untouched; on a
 * time-ordered row head 1's second pass starts from the quotients the bar's mask left.
 *   pb_batch_decoder_schedule       in pb_batch_decoder_allow's window and after it (the masks every schedule points to go up with the rows'
 *                                   masks in that ONE call): table = (n_sched, nbar) host ints, nbar = pad[0]; row_sched = (B) host ints, the
 *                                   index of row b's schedule, -1 = none (what sampler_init sets for every row). The table is copied to
 *                                   device memory the decoder owns; the indices are stored beside the rows' mask indices in decoder-stream
 *                                   order; pb_batch_decoder_start keeps them. Same kernels, kernarg layouts and launches per step. Refused
 *                                   (< 0, pb_last_error, nothing changed): a null argument, before sampler_init, after a step was issued or
 *                                   captured, n_sched < 1, nbar != pad[0], an entry outside -1 .. n_masks - 1, a row index outside -1 ..
 *                                   n_sched - 1. While a schedule is in place pb_batch_decoder_allow is refused (the entries point into its
 *                                   table); a later sampler_init clears both.
 *   pb_batch_decoder_admit_schedule refill: stages the schedule index (-1 .. n_sched - 1 of the table pb_batch_decoder_schedule uploaded, which
 *                                   therefore holds the schedules of ALL rows of the call from the start) that the next
 *                                   pb_batch_decoder_admit of `row` stores, with the row's mask index. An admit without a staged value
 *                                   stores -1: a slot never inherits its previous occupant's schedule. Host state only. Refused (< 0,
 *                                   pb_last_error, nothing changed): not a dynamic decoder, before sampler_init, row outside 0 .. B - 1, an
 *                                   index outside the table. */
#define PB_DECODE_BATCH_MAX 16
typedef struct pb_decode_batch {
    pb_decode_plan plan;
    int32_t B; int32_t _pad;
    int32_t s_enc[PB_DECODE_BATCH_MAX];
} pb_decode_batch;
int pb_batch_decoder_create(const pb_decode_batch* plan, void** dec);
int pb_batch_decoder_destroy(void* dec);
int pb_batch_decoder_reset(void* dec, void* caller_stream, int32_t use_graph);
int pb_batch_decoder_step(void* dec, const int16_t* tok8, float* logits_out);
int pb_batch_decoder_sampler_init(void* dec, const float* temps8, const float* p8, const int32_t* n8, const int32_t* off8, const int32_t* pad8,
                                  const double* u, int64_t n_u, int32_t limit, int32_t fault_row, int32_t fault_period);
int pb_batch_decoder_launch(void* dec, int32_t ntok, const int16_t* first_tok);
int pb_batch_decoder_wait(void* dec, int32_t ticket);
int pb_batch_decoder_logs(void* dec, float** logits_rows, int16_t** tok_rows);
int pb_batch_decoder_seek(void* dec, int32_t row, int32_t pos, const int16_t* tok8);
int pb_batch_decoder_start(void* dec, const int32_t* last_pos, const int16_t* next_tok, const int32_t* limit);
int pb_batch_decoder_launches(void* dec);
int pb_batch_decoder_graph(void* dec);
int pb_batch_decoder_share_cross(void* dec, int32_t n_groups, const int32_t* kv_row);
int pb_batch_decoder_force(void* dec, const int16_t* forced);
int pb_batch_decoder_dynamic(void* dec, int32_t n_slices);
int pb_batch_decoder_admit(void* dec, int32_t row, int32_t slice, int32_t s_enc, int32_t last_pos, const int16_t* next_tok8, int32_t limit,
                           const double* u_row, const int16_t* forced_row, const float* mask_row, void* caller_stream);
int pb_batch_decoder_fence(void* dec, void* caller_stream);
int pb_batch_decoder_stop(void* dec, const int32_t* stop_bar);
int pb_batch_decoder_admit_stop(void* dec, int32_t row, int32_t stop_bar);
int pb_batch_decoder_order(void* dec, const int32_t* floor);
int pb_batch_decoder_admit_order(void* dec, int32_t row, int32_t floor);
int pb_batch_decoder_sampler_form(void* dec);
int pb_batch_decoder_allow(void* dec, const uint32_t* masks, int32_t n_masks, int32_t words, const int32_t* row_mask);
int pb_batch_decoder_admit_allow(void* dec, int32_t row, int32_t mask_index);
int pb_batch_decoder_schedule(void* dec, const int32_t* table, int32_t n_sched, int32_t nbar, const int32_t* row_sched);
int pb_batch_decoder_admit_schedule(void* dec, int32_t row, int32_t sched_index);
/* Anchored notes (an addition to ABI 10): a row may carry a list of anchors, complete tokens A[0 .. n) of 8 ordinary ids in non-decreasing
 * (bar, position) order, and a counter k of those written (0 at start and admit). Every position is sampled as without them -- the
 * candidate c, under the row's floor, mask, schedule and draws -- and the sampler's last stage decides: if k < n and (c ends the row: c[0]
 * >= the row's stop bar or a special id in any head; or (c[0], c[1]) >= (A[k][0], A[k][1])) the 8 ids written are A[k], k becomes k + 1
 * and the row is NOT done; else c is written and the done test is what it was. Both forms and both widths of the sampler, the kernels
 * without the force table; the caller makes an anchored row time-ordered (pb_batch_decoder_order, floor >= 0).
 *   pb_batch_decoder_anchor         between sampler_init and start, behind pb_batch_decoder_stop / _order: rows = (n_rows, 8) host ids, the
 *                                   anchors of ALL rows of the call, copied to device memory the decoder owns; row_base / row_cnt = (B) host
 *                                   ints, row b's anchors are rows row_base[b] .. + row_cnt[b] - 1 (count 0 = none). Stored in
 *                                   decoder-stream order; pb_batch_decoder_start keeps them and sets the counters to 0. Same kernels, kernarg
 *                                   layouts and launches per step. Refused (< 0, pb_last_error, nothing changed): a null argument, before
 *                                   sampler_init, after a step was issued or captured, a decoder with a force table (and pb_batch_decoder_force
 *                                   is refused behind it), n_rows < 1, a slice outside the table, more anchors than S, an id outside 0 ..
 *                                   pad[h] - 1, a row's anchors out of (bar, position) order, a bar below the row's floor or >= its stop bar.
 *   pb_batch_decoder_admit_anchor   refill: stages the slice of that table the next pb_batch_decoder_admit of `row` stores, with a counter
 *                                   of 0; behind the row's admit_stop / admit_order. An admit without a staged value stores none: a slot
 *                                   never inherits its previous occupant's anchors. Host state only. Refused: not a dynamic decoder, before
 *                                   sampler_init, row outside 0 .. B - 1, a slice outside the table, order or bars as above.
 *   pb_batch_decoder_seek_anchor    with the pb_batch_decoder_seek that rewinds `row`: sets its counter to `placed`, the number of anchors
 *                                   the host has written up to the position sought, in decoder-stream order. Refused: before sampler_init,
 *                                   row outside 0 .. B - 1, placed outside 0 .. the row's count.
 *   pb_batch_decoder_anchors_placed drains what is enqueued and reads the B counters into out (0 for a row without anchors). */
int pb_batch_decoder_anchor(void* dec, const int16_t* rows, int32_t n_rows, const int32_t* row_base, const int32_t* row_cnt);
int pb_batch_decoder_admit_anchor(void* dec, int32_t row, int32_t base, int32_t cnt);
int pb_batch_decoder_seek_anchor(void* dec, int32_t row, int32_t placed);
int pb_batch_decoder_anchors_placed(void* dec, int32_t* out);

/* ---- K15: deferred parameter-gradient reductions -----------------------------------------------------------------------
 * The bias / LayerNorm-parameter gradients of one backward pass (the `db = grad.sum(0)` of every nn.Linear and nn.LayerNorm autograd
 * node under BartModel, modeling_bart.py:280-390) leave their kernels as per-workgroup partial rows. Between pb_defer_begin and
 * pb_defer_flush (same host thread) pb_add_ln_bwd, pb_gemm (colsum_out) and pb_attn_bwd (dbias_*) keep those rows in `arena`
 * instead of reducing them one small launch at a time, and pb_defer_flush sums all of them in ONE launch, in a fixed order
 * (bit-reproducible). arena: device floats, 16-byte aligned; table: device bytes, table_entries * pb_defer_desc_bytes(). When either
 * is full the calls fall back to the immediate reduction. Outputs are accumulated (+=) exactly as without deferral, so they must
 * not be read, nor written by anything else, before the flush. */
int pb_defer_begin(float* arena, int64_t arena_floats, void* table, int32_t table_entries);
int pb_defer_flush(void* stream);

/* ---- events for ordering two streams of one GPU (Engine's second stream) ---------------------------
 * mode bit 0: hipEventDisableSystemFence, bit 1: hipEventReleaseToDevice (both on top of hipEventDisableTiming): the producer and
 * the consumer are kernels on the same device, so the system-scope write-back / invalidate of a default event is not needed.
 * The handle is an opaque hipEvent_t. */
int pb_event_create(void** ev, int32_t mode);
int pb_event_destroy(void* ev);
int pb_event_record(void* ev, void* stream);
int pb_stream_wait_event(void* stream, void* ev);
int32_t pb_defer_desc_bytes(void);

/* ---- K27: LoRA, low-rank adapters on the attention projections (pb_lora.hip; additions to ABI 10) ------------------------
 * y = x W^T + b + s (x A^T) B^T with A (r, K), B (N, r), s = alpha / r (DESIGN.md 5 "LoRA"). The activations X / Y are rows of the storage
 * dtype (PB_BF16 or PB_F32) with a leading dimension ld and a column offset, both in elements (the q / k / v slice of a (T, 3d) buffer is
 * ld = 3d, offset 0 / d / 2d); they are read or written once, with 16-byte vectors where the slice's address and ld allow them. The adapter
 * matrices, T and all sums are f32 (f32-input MFMA: an f32 fma chain). r is a multiple of 4 in 4 .. 64; 0 <= M <= 2^24 and M = 0 returns 0
 * without a launch. No atomics: equal inputs give equal bytes. Every entry checks its arguments before the first HIP call (-2,
 * pb_last_error names the argument).
 *
 * pb_lora_down:  T (M, r) = alpha * X (M, K) * W^T. w_kr = 0: W is (r, K); 1: W is (K, r). pb_lora_down_rows() rows per workgroup.
 * pb_lora_up:    Y (M, N) += alpha * T (M, r) * W, a read-modify-write in Y's dtype (one rounding). w_nr = 0: W is (r, N); 1: W is (N, r).
 *                Nothing outside columns y_off .. y_off + N - 1 of rows 0 .. M - 1 is written. pb_lora_up_rows() rows per workgroup.
 * pb_lora_wgrad: G = alpha * T (M, r)^T * X (M, C), overwritten. g_cr = 0: G is (r, C); 1: G is (C, r). M is cut into
 *                pb_lora_wgrad_chunk(M, r) rows per wave, each wave writes its partial to its slot of ws (pb_lora_wgrad_ws_floats(M, r, C) floats,
 *                16-byte aligned; 0 for sizes the entry refuses) and the slots are added in slot order.
 * pb_lora_merge: W (N, K) += alpha * B (N, r) A (r, K), all f32 with dense rows: an fma chain over r per element and one fma onto W. */
int pb_lora_down_rows(void);
int pb_lora_up_rows(void);
int64_t pb_lora_wgrad_chunk(int64_t M, int32_t r);
int64_t pb_lora_wgrad_ws_floats(int64_t M, int32_t r, int32_t C);
int pb_lora_down(const void* X, int64_t ldx, int64_t x_off, int32_t dtype, const float* W, int32_t w_kr, float* T, int64_t M, int32_t K, int32_t r,
                 float alpha, void* stream);
int pb_lora_up(void* Y, int64_t ldy, int64_t y_off, int32_t dtype, const float* T, const float* W, int32_t w_nr, int64_t M, int32_t N, int32_t r,
               float alpha, void* stream);
int pb_lora_wgrad(const float* T, const void* X, int64_t ldx, int64_t x_off, int32_t dtype, float* G, int32_t g_cr, int64_t M, int32_t C, int32_t r,
                  float alpha, float* ws, void* stream);
int pb_lora_merge(float* W, const float* B, const float* A, int64_t N, int32_t K, int32_t r, float alpha, void* stream);

#ifdef __cplusplus
}
#endif
#endif

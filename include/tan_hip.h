/* tan_hip.h -- C ABI of libtan_hip.so: the MI355X (gfx950) kernels behind the TemporalAlignNet hot path.
 *
 * The reference (TengdaHan/TemporalAlignNet) is pure Python and has no FFI layer of its own: its seam is
 * the nn.Module surface of model/tan_model.py + train/loss.py:get_loss, and every arithmetic op below that
 * seam is a PyTorch ATen call.  Each entry point here replaces the ATen kernels behind one reference call
 * site (cited per function as reference file:line).  temporalalignnet_amd/_lib.py binds them with ctypes;
 * INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *  - plain pointers + sizes, no torch types; all pointers are DEVICE pointers unless stated otherwise.
 *  - `stream` is a hipStream_t passed as void*; every call only enqueues work on it (no allocation, no
 *    synchronisation, no global state) and is safe to capture into a hipGraph.
 *  - return 0 on success, a hipError_t value, or TAN_ERR_BAD_ARG (-1) for an invalid argument.
 *  - `dtype` selects the activation type: TAN_F32 (parity mode, exact-f32 MFMA) or TAN_BF16 (throughput
 *    mode, bf16 operands, f32 accumulation).  Statistics, logits, losses and parameter gradients are f32.
 *  - activations are batch-first, row = b*L + t, channels contiguous.
 */
#ifndef TAN_HIP_H
#define TAN_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define TAN_F32 0
#define TAN_BF16 1
#define TAN_ERR_BAD_ARG (-1)

#define TAN_ACT_NONE 0
#define TAN_ACT_QUICKGELU 1      /* C = x*sigmoid(1.702x), x = acc+bias; x itself optionally stored to aux */
#define TAN_ACT_QUICKGELU_GRAD 2 /* C = acc * d/dx quickgelu(x), x read from aux */
#define TAN_ACT_RELU 3           /* C = max(acc+bias, 0)  (Word2VecModel fc1, model/word2vec_model.py:86) */

int tan_version(void);          /* 110: tan_compound_topk / _peaks; 109: tan_chapter_costs / _decode; 108: tan_storyboard_select; 107: tan_cover_topk / _e4m3; 106: tan_quantize_rows_mxfp4 / tan_rank_topk_mxfp4; 105: tan_cluster_accumulate / _centroids; 104: tan_local_align_path; 103: tan_local_align; 102: tan_label_decode; 101: tan_clip_topk / _e4m3 (100: everything before them) */
/* sizeof(tan_gemm_desc | tan_layer_params | tan_layer_bufs | tan_encoder_desc | tan_simfam_desc | tan_simnce_desc) for which = 0..5 (binding self-check) */
int tan_abi_sizeof(int which);

/* Optional in-stream kernel timer (bench.py's `roofline` line): while enabled every tan_gemm / tan_attn_* launch is
 * bracketed by hipEvents on its own stream.  tan_prof_collect synchronises and returns per kind the summed duration
 * [ms], the summed ALGORITHMIC work [flop] (2*M*N*K per GEMM; 4*B*H*L*L*64 attention fwd, 14*... bwd incl. recompute)
 * and the launch count; returns 1 if the record buffer overflowed.  tan_prof_enable: on = 1 starts a fresh recording,
 * on = 0 pauses it (records are kept), on = 2 resumes -- bench.py samples every 4th timed step this way.  GEMM kinds: base + 2*(A K-strided) + (B K-strided). */
#define TAN_PROF_GEMM_BF16 0
#define TAN_PROF_GEMM_F32 4
#define TAN_PROF_ATTN_FWD 8
#define TAN_PROF_ATTN_BWD 9
#define TAN_PROF_SIMNCE 10
#define TAN_PROF_PANEL 11   /* row-panel fused MLP kernels (tan_mlp_fwd / tan_mlp_bwd) */
#define TAN_PROF_ATTNBLK 12 /* the attention branch of a block in one launch (tan_attnblk_*) */
#define TAN_PROF_NKINDS 13
int tan_prof_enable(int on, int max_records);
/* time only every stride-th eligible launch from now on (1 = all): a sample of the launches instead of each of them */
int tan_prof_stride(int stride);
/* work [flop] and launch count of EVERY eligible launch since tan_prof_enable(1, ..) / the last call (timed or not); resets them */
int tan_prof_collect_all(double* work_by_kind, long* count_by_kind, int nkinds);
int tan_prof_collect(double* ms_by_kind, double* work_by_kind, long* count_by_kind, int nkinds);

/* Stream-ordering events (no timing) for tan_encoder_desc.layer_done: the reference's DDP (end2end/main_nce.py:142-158) hooks
 * autograd to start reducing a gradient bucket while backward continues; here one call runs a whole stack's backward, so the
 * library records an event per layer and the caller makes its communication stream wait for it. */
int tan_event_create(void** event);
int tan_event_destroy(void* event);
int tan_stream_wait_event(void* stream, void* event);

/* ---- GEMM (nn.Linear fwd/bwd: tfm_model.py:21-27, tan_model.py:48-49,70; einsum tan_model.py:118,138) ----
 * C[M,N] (=|+=) alpha * opA(A)[M,K] * opB(B)[K,N]  (+ bias[N]) (activation) (+ residual[M,N])
 *   a_kc=1: A stored [M,K] (lda = row stride)   a_kc=0: A stored [K,M] (lda = stride between k)
 *   b_kc=1: B stored [N,K] ("x @ W^T")          b_kc=0: B stored [K,N]
 * Operands are `dtype`, C/residual/aux are `out_dtype`.  accumulate=1 (requires out_dtype F32, no
 * bias/act/residual) adds into C with f32 atomics and allows split_k > 1.  Batched over `batch` with
 * element strides sA/sB/sC (residual and aux share sC).                                                  */
typedef struct tan_gemm_desc {
    int dtype, out_dtype;
    int M, N, K;
    int a_kc, b_kc;
    const void* A; long lda;
    const void* B; long ldb;
    void* C; long ldc;
    const float* bias;
    const void* residual; long ldr;
    int act;
    void* aux; long ldaux;
    int accumulate;
    int split_k;
    float alpha;
    int batch; long sA, sB, sC;
    float* colsum; /* optional [N] f32: += column sums of the stored elements of C (fused bias gradient; rows ldc apart); batch must be 1.
                      A bf16 C whose epilogue is vectorised (N % 8 == 0, 16-byte aligned C / residual / aux rows) adds the f32 values
                      BEFORE the rounding of the store; every other path adds the values it reads back from C */
} tan_gemm_desc;
int tan_gemm(const tan_gemm_desc* d, void* stream);

/* ---- LayerNorm(C), eps, affine; one wave per row; C in {256,512,1024} -------------------------------------
 * fwd: y = (x-mean)*rstd*gamma+beta (+ add[row % add_period], the broadcast position term of
 *      tan_model.py:167,199).  reference: tfm_model.py:22,28,35,37; tan_model.py:50-54,155,174,206.
 *      mean/rstd [rows] f32 are saved for backward (may be NULL).
 * bwd: dx = (dres +) LN'(dy); dgamma/dbeta (f32, may be NULL) are ACCUMULATED (+=); dx_colsum (may be NULL) += column
 *      sums of the OUTPUT dx, i.e. the bias gradient of the Linear that wrote the stream this LN normalises (saves a
 *      separate pass).  ws: f32 scratch of tan_layernorm_bwd_ws_floats(C) elements.                           */
int tan_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                      const void* add, int add_period, long rows, int C, float eps, int dtype, void* stream);
long tan_layernorm_bwd_ws_floats(int C);
int tan_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                      const void* dres, void* dx, float* dgamma, float* dbeta, float* dx_colsum, float* ws, long rows, int C,
                      int dtype, void* stream);

/* ---- L2 normalisation over channels, no epsilon (tan_model.py:116-117,136-137) ---------------------------
 * Output rows r = 0..rows-1 are gathered from x row (r/grp)*src_grp_rows + src_off + r%grp, which extracts the
 * video rows (off 0, grp T) or the text rows (off T, grp N) of a joint [B, T+N, C] stage output; bwd scatters
 * dx = (dy - y<y,dy>) * inv_norm back to the same rows (plain store).                                        */
int tan_l2norm_fwd(const void* x, void* y, float* inv_norm, long rows, int C, int grp, int src_grp_rows, int src_off,
                   int dtype, void* stream);
int tan_l2norm_bwd(const void* dy, const void* y, const float* inv_norm, void* dx, long rows, int C, int grp,
                   int dst_grp_rows, int dst_off, int dtype, void* stream);
/* The same for up to 8 deep-supervision stages in ONE launch (tan_model.py:116-117,136-137 run per stage of the [B,S,T,C]
 * features): stage s reads / scatters to its own buffer xs->p[s] / dxs->p[s]; y, dy [nstage][rows][C] and inv_norm
 * [nstage][rows] are stage-major contiguous.                                                                             */
typedef struct tan_ptr8 { const void* p[8]; } tan_ptr8;
int tan_l2norm_fwd_multi(const tan_ptr8* xs, void* y, float* inv_norm, int nstage, long rows, int C, int grp,
                         int src_grp_rows, int src_off, int dtype, void* stream);
int tan_l2norm_bwd_multi(const void* dy, const void* y, const float* inv_norm, const tan_ptr8* dxs, int nstage, long rows,
                         int C, int grp, int dst_grp_rows, int dst_off, int dtype, void* stream);

/* ---- small HBM-bound helpers ----------------------------------------------------------------------------- */
/* out[c] += sum_r x[r][c]  (nn.Linear bias gradients) */
int tan_colsum_acc(const void* x, float* out, long rows, int C, int dtype, void* stream);
/* dst[(g*dst_grp_rows+dst_off+r)][c] (=|+=) src[(g*src_grp_rows+src_off+r)][c], g<G, r<R  (torch.cat at
 * tan_model.py:201 and its backward split) */
int tan_rows_copy(const void* src, void* dst, int G, int R, int C, long src_grp_rows, long src_off, long dst_grp_rows,
                  long dst_off, int accumulate, int dtype, void* stream);
/* dst[s][m][:] = map[m] >= 0 ? src[s][map[m]][:] : 0, s < S  (src [S, Msrc, C], dst [S, Mdst, C], map int32 [Mdst]): the compacted
 * text-feature gradient of the logits-free NCE back in the padded [B*N] row order -- torch.zeros().index_copy_() in one launch */
int tan_rows_gather(const void* src, void* dst, const int* map, int S, long Msrc, long Mdst, int C, int dtype, void* stream);
/* out[r][c] = sum_g x[g*R + r][c]  (backward of the broadcast position add) */
int tan_group_sum(const void* x, void* out, int G, int R, int C, int dtype, void* stream);
int tan_cast(const void* src, int src_dtype, void* dst, int dst_dtype, long n, void* stream);
/* y = x * sigmoid(1.702 x): QuickGELU.forward called on its own (model/tfm_model.py:11-13); in a block it is a GEMM epilogue */
int tan_quickgelu(const void* x, void* y, long n, int dtype, void* stream);
/* out[i] += sum_s parts[s*n + i]  (folds split-K partial tiles into an f32 gradient); n % 4 == 0 */
int tan_reduce_add(const float* parts, float* out, int nparts, long n, void* stream);
/* Batched bf16 transpose inside one flat buffer: matrix i is src[table[3i] ...] with shape [table[3i+1], table[3i+2]] (row-major;
 * both multiples of 8, offsets multiples of 8); dst gets its transpose at the same element offset.  `table` is DEVICE memory.
 * Produces the K-contiguous weight copies tan_layer_params.wt_* (dX = dY W reads W^T rows) once per optimizer step.        */
int tan_transpose_batch(const void* src, void* dst, const long* table, int n, long max_rows, long max_cols, int dtype,
                        void* stream);
/* binary_head = nn.Linear(512,1) (tan_model.py:70,147-148): out[r] = <x[r],w> + b (f32 out); bwd accumulates dw, db */
int tan_head_fwd(const void* x, const float* w, const float* b, float* out, long rows, int C, int dtype, void* stream);
int tan_head_bwd(const float* dout, const void* x, const float* w, void* dx, float* dw, float* db, long rows, int C,
                 int accumulate_dx, int dtype, void* stream);
/* F.interpolate(mode='linear', align_corners=False) of a [L_in,C] f32 table (tan_model.py:157-160,189-192); bwd adds */
int tan_interp_linear(const float* src, float* dst, int L_in, int L_out, int C, void* stream);
int tan_interp_linear_bwd(const float* ddst, float* dsrc, int L_in, int L_out, int C, void* stream);

/* ---- attention core: softmax_k(q k^T / sqrt(64) + key_padding) v per (video, head) -------------------------
 * replaces the scaled-dot-product inside nn.MultiheadAttention (tfm_model.py:21,30-32); head dim 64, C = 64*H.
 * qkv [B*L, 3C] (output of the packed in-proj GEMM, q|k|v), key_padding_mask [B,L] bytes (1 = ignore) or NULL,
 * o [B*L, C], lse [B,H,L] f32 (saved for backward).  bwd recomputes P from lse and writes dqkv [B*L, 3C].
 * L <= 448 (f32) / 320 (bf16): the score panel of a 64-query tile lives in the 160 KB LDS.                      */
int tan_attn_fwd(const void* qkv, const unsigned char* key_padding_mask, void* o, float* lse, int B, int L, int H,
                 int dtype, void* stream);
int tan_attn_bwd(const void* qkv, const unsigned char* key_padding_mask, const void* o, const float* lse,
                 const void* d_o, void* dqkv, int B, int L, int H, int dtype, void* stream);
/* the same, and g_b_qkv [3C] f32 += column sums of dqkv (the in_proj bias gradient of nn.MultiheadAttention): summed in
 * the backward kernel from the rows it is about to store when L <= 128 (bf16), by tan_colsum_acc over dqkv otherwise    */
int tan_attn_bwd_bias(const void* qkv, const unsigned char* key_padding_mask, const void* o, const float* lse,
                      const void* d_o, void* dqkv, float* g_b_qkv, int B, int L, int H, int dtype, void* stream);

/* ---- loss side (train/loss.py:get_loss) -------------------------------------------------------------------
 * logits: raw cosines, stage-major [S, R=B*T, Mp=B*N] f32 (the reference's [B,S,T,B,N] is a permuted view).
 * tgt [B,T,N] f32 {0,1}: same-video targets (loss.py:73-76 or the self-labelled ones, loss.py:227);
 * col_invalid [Mp] bytes: padded texts (dropped columns, loss.py:233,241); row_leak [R] bytes or NULL: frames whose
 * same-video logits read -6e4 (reference in-place quirk for model='init' + learn_agreement, loss.py:96-101).
 *
 * tan_nce_fwd: symmetric multi-positive NCE terms of loss.py:240-253 (and 262-274):
 *   v_terms[s,r] = LSE_cols(all) - LSE_cols(pos), t_terms[s,c] = LSE_rows(all) - LSE_rows(pos); the row/column sums of
 *   exp(l/0.07 - 1/0.07) are saved (rowsum [S,R], colsum [S,Mp], possum_v [S,R], possum_t [S,Mp]) for tan_nce_bwd, which
 *   turns upstream g_v [S,R], g_t [S,Mp] into dlogits [S,R,Mp] (out_dtype).  ws: tan_nce_ws_floats() f32 scratch.
 *   A row with an empty positive set takes the reference's fill -6e4 + log(#real text columns): n_valid_cols when > 0, else
 *   counted from col_invalid on the device (the fused sweeps always count their col_invalid that way).                */
long tan_nce_ws_floats(int S, int B, int T, int N);
int tan_nce_fwd(const float* logits, const float* tgt, const unsigned char* col_invalid, const unsigned char* row_leak,
                float* rowsum, float* colsum, float* possum_v, float* possum_t, float* v_terms, float* t_terms, float* ws,
                int S, int B, int T, int N, int n_valid_cols, void* stream);
int tan_nce_bwd(const float* logits, const float* tgt, const unsigned char* col_invalid, const unsigned char* row_leak,
                const float* rowsum, const float* colsum, const float* possum_v, const float* possum_t, const float* g_v,
                const float* g_t, void* dlogits, int out_dtype, int S, int B, int T, int N, void* stream);
/* `blocks`: the last-stage same-video logit blocks; element (b,t,n) at blocks[b*block_stride + t*row_stride + n].  For
 * materialised stage-major logits: blocks = logits + (S-1)*R*Mp, block_stride = T*Mp + N, row_stride = Mp; for a compact
 * [B,T,N] tensor: T*N and N.
 * self-labelling scan, loss.py:88-143 (joint) / 146-179 (dual): two-way softmax (over texts, /0.07, over time) of the
 * last-stage same-video logits, sliding-window mean with window length dur[b,n] (0 = padded text), first-index argmax.
 * Outputs max_pos [B,N] int32, max_prob/max_logit [B,N] f32, self_tgt [B,N,T] bytes (the chosen window).            */
int tan_selflabel(const float* blocks, long block_stride, long row_stride, const unsigned char* video_pad,
                  const unsigned char* text_pad, const float* dur, int* max_pos, float* max_prob, float* max_logit,
                  unsigned char* self_tgt, int B, int T, int N, void* stream);
/* out[b,n] = max_t block(b,t,n) / 0.07   (loss.py:280,283) */
int tan_diag_max(const float* blocks, long block_stride, long row_stride, const unsigned char* row_leak, float* out, int B, int T,
                 int N, void* stream);
/* IoU of the two self-labelled windows, confidence, target policy kind (0 'i', 1 'u', 2 'keep', 3 'keep-joint') and the
 * per-frame first-text de-duplication with restore, loss.py:181-226.  q_joint/q_dual: device scalars (0.3-quantiles of
 * the max logits).  tgt_out [B,T,N] f32, iou [B,N] f32, conf [B,N] bytes.  N <= 64.                                 */
int tan_agreement(const unsigned char* joint_tgt, const unsigned char* dual_tgt, const unsigned char* youtube_tgt,
                  const float* max_logit_joint, const float* max_logit_dual, const float* q_joint, const float* q_dual,
                  int kind, float* tgt_out, float* iou, unsigned char* conf, int B, int T, int N, void* stream);
/* torch.quantile(x[~invalid], q) ('linear' interpolation, at::lerp rounding) without a host sync; n <= 8192 */
int tan_masked_quantile(const float* x, const unsigned char* invalid, int n, float q, float* out, void* stream);

/* ---- logits-free similarity + NCE (bf16 features) ---------------------------------------------------------------
 * Fused replacement of einsum (tan_model.py:118,138) + NCE terms (loss.py:240-253) and of their autograd: one workgroup sweeps a
 * 128-row panel of one stage over all text columns; logits only ever exist as MFMA accumulators.  Both calls take one descriptor;
 * tgt / col_invalid / row_leak and the four saved sums mean what they mean for tan_nce_fwd.  Requires C % 64 == 0 and at most
 * tan_simnce_max_cols() sweep columns.
 *   tan_simnce_fwd  row / column / positive sums and v_terms [S,R], t_terms [S,Mp].  e_keep != NULL (tan_simnce_keeps(C) != 0: the
 *                   LDS-resident sweep, C = 512) also stores e = exp((cos - 1)/tau) of every (frame, sentence) pair as bf16,
 *                   tan_simnce_keep_elems() elements: S * ceil(R/128) * ceil(Mp/128) tiles of 128 x 128 in accumulator order.
 *   tan_simnce_bwd  g_v [S,R], g_t [S,Mp] -> dl = d loss/d logits [S,R,Mp] bf16 for the follow-up tan_gemm calls.  e_keep NULL: a
 *                   second sweep recomputes the logits; e_keep != NULL: one element-wise pass over the kept exponentials (2 x
 *                   S*R*Mp*2 bytes of HBM traffic instead of 2*S*R*Mp*C FLOP).  d_vn != NULL (needs e_keep, TAN_SIM_SWEEP, C = 512,
 *                   16-byte alignment, sweep columns % 8 == 0 and < 32768, N <= 32): that pass also returns d_vn [S,R,C] bf16 =
 *                   dl . t_hat, the gradient of the unit video features (autograd of tan_model.py:116-119,136-139's einsum towards
 *                   its first operand) -- the 128 x 128 d-logits tiles are the MFMA operand while they are in the LDS, so the
 *                   [S*R, Mp] x [Mp, C] GEMM and its read of dl go away.  dl is still written for the text-feature gradient (NULL:
 *                   not written); the sweep's text image inside `ws` is overwritten and (unless TAN_SIM_CORR_KEEP) the dense
 *                   same-video correction array is built there.
 * Column compaction (colmap != NULL; NULL: Mc is ignored): padded text columns take part in nothing (loss.py:64-70 drops them before
 * the log-sum-exps), so the sweep may run on a COMPACTED text matrix: `tn` then holds Mc <= B*N rows per stage (a multiple of 64 keeps
 * the follow-up GEMMs on the direct-to-LDS kernel; filler rows flagged in col_invalid), col_invalid / colsum / possum_t / t_terms / g_t
 * have Mc entries per stage, dl is [S,R,Mc]; `tn_blocks` is the UNcompacted [B*N,C] matrix, read only for the same-video blocks, and
 * colmap[b*N+k] is that sentence's compacted column or -1.
 * `phases` (0 = everything) selects the steps, for sweeps over SEVERAL column blocks (global negatives across ranks, row f3):
 *   TAN_SIM_SWEEP  the tile sweep (fwd: row sums += valid columns, column sums of this block -> colsum; bwd: d logits)
 *   TAN_SIM_ACC_ROWS  with SWEEP: keep accumulating into rowsum instead of zeroing it first
 *   TAN_SIM_DIAG   same-video blocks: positives + padded-frame quirk (only the block that holds the rows' own sentences)
 *   TAN_SIM_TERMS  (fwd) v_terms / t_terms from the final sums
 *   TAN_SIM_DIAG_KEEP  (bwd, with DIAG) `ws` still holds the same-video blocks tan_simnce_fwd computed for these features: do
 *                  not recompute them
 *   TAN_SIM_CORR_KEEP  (bwd, d_vn != NULL) `ws` already holds the correction array of these upstream gradients                  */
#define TAN_SIM_SWEEP 1
#define TAN_SIM_DIAG 2
#define TAN_SIM_TERMS 4
#define TAN_SIM_ACC_ROWS 8
#define TAN_SIM_DIAG_KEEP 16
#define TAN_SIM_CORR_KEEP 32
typedef struct tan_simnce_desc {
    int S, B, T, N, C, Mc, phases;
    const void* vn;                                    /* [S,R,C] unit video features, R = B*T */
    const void* tn; long t_stage_stride;               /* [S or 1,Mp,C] unit text features; Mp*C, or 0: shared by all stages */
    const void* tn_blocks; long tb_stage_stride;       /* with colmap: the uncompacted text features and their stage stride */
    const int* colmap;                                 /* [B*N] or NULL */
    const float* tgt; const unsigned char* col_invalid; const unsigned char* row_leak;   /* [B,T,N] | [Mp] | [R] or NULL */
    float *rowsum, *colsum, *possum_v, *possum_t;      /* [S,R], [S,Mp], [S,R], [S,Mp]: written by fwd, read by bwd */
    float *v_terms, *t_terms;                          /* fwd out */
    const float *g_v, *g_t; void* dl; void* d_vn;      /* bwd: in, in, out, optional out */
    void* e_keep;                                      /* optional: kept exponentials, written by fwd, read by bwd */
    float* ws;                                         /* tan_simnce_ws_floats() f32 scratch */
} tan_simnce_desc;
long tan_simnce_ws_floats(int S, int B, int T, int N);
int tan_simnce_max_cols(void);   /* most text columns (B*N, or Mc when compacted) one sweep accepts: callers fall back to tan_nce_* above it */
int tan_simnce_keeps(int C);     /* != 0: tan_simnce_fwd can keep its exponentials for C channels */
long tan_simnce_keep_elems(int S, int R, int Mp);
int tan_simnce_fwd(const tan_simnce_desc* d, void* stream);
int tan_simnce_bwd(const tan_simnce_desc* d, void* stream);

/* ---- one feature FAMILY (dual or joint) of the logits-free NCE, from the stacks' stage outputs to their gradients --------------
 * Everything between an encoder stack's forward and its backward in the training step, for one family of tan_model.py:116-119
 * (dual: video stack stages x the one text embedding) or :136-139 (joint: video rows x text rows of the joint stack's stages), with
 * loss.py:240-253 and its autograd:
 *   tan_simfam_fwd  L2-normalise the stage rows (video: one launch, or inside the sweep's panel load with TAN_SIMFAM_NORM_IN_SWEEP;
 *                   text: normalise + column compaction + both fragment-major text images in ONE launch), the statistics sweep keeping
 *                   its exponentials (tan_simnce_fwd's kernel, e_keep set), and ONE finishing launch: same-video cosine blocks, column sums
 *                   over the row panels, positives / leaked frames, v_terms / t_terms -- and, when g_v / g_t are already known (the
 *                   two-chain step: they depend on the batch's masks only), the same-video corrections of the backward.
 *   tan_simfam_bwd  d logits + d v_hat in one pass over the kept exponentials whose epilogue applies the L2-normalisation's backward
 *                   and stores straight into the stacks' stage-gradient rows (d v_hat never exists in HBM); the text-feature gradient
 *                   GEMM d t_hat = dl^T v_hat (f32, split-K); one launch that gathers it back to the padded sentence order, applies
 *                   the normalisation's backward and stores the text stage-gradient rows.
 * 6-7 launches per family and step instead of 18.  bf16, C = 512, N <= 32, Mc % 8 == 0, Mc <= tan_simnce_max_cols(), S <= 8.
 * Row addressing: video row r = b*T + t of stage s lives at x_video.p[s] + ((r / T) * v_grp_rows + v_off + r % T) * C (video stack:
 * v_grp_rows = T; joint stack: T + N); padded sentence m = b*N + k at x_text.p[st] + ((m / N) * t_grp_rows + t_off + m % N) * C;
 * d_video / d_text are addressed the same way.  St = 1: one text embedding for all stages (dual), St = S: per stage (joint).
 * Column compaction as tan_simnce_fwd: idx [Mc] (sweep column -> padded sentence), colmap [B*N] (or both NULL: Mc = B*N, identity).
 * Sweep column c holds the unit row of padded sentence idx[c], filler columns (flagged in col_invalid) included; their t_terms are
 * finite and meaningless.  The [T, N] block the finishing launch holds twice in the LDS bounds T: 8*T*N + 5*T + 1584 <= 163840 bytes
 * (T <= 621 at N = 32), checked with everything else before the first launch of either call.
 * row_leak: a flagged frame gets its terms by SUBTRACTING its same-video exponentials from the sweep's row and column sums.  That
 * needs the other videos' part to stay above about 1e-4 of the sum (f32); with B = 1, or when every other video's cosine to the frame
 * is far below its same-video ones (two or three videos at cosines < -0.4 against 0.9), the terms of flagged frames and of padded
 * columns are rounding noise or non-finite.  Callers with such batches take tan_nce_fwd on materialised logits.
 * Saved between the two calls (caller-owned): vn [S,R,C], inv_v [S,R], tn [St,Mc,C], inv_t [St,Mc], rowsum / possum_v [S,R],
 * colsum / possum_t [S,Mc], e_keep (tan_simnce_keep_elems), ws (tan_simfam_ws_bytes).                                              */
#define TAN_SIMFAM_NORM_IN_SWEEP 1   /* flags: the sweep normalises its frame panel itself and writes vn / inv_v (no separate launch) */
#define TAN_SIMFAM_CORR_DONE 2       /* (set by tan_simfam_fwd when g_v / g_t were given) ws holds the corrections: bwd skips that launch */
/* tan_simfam_fwd in two calls, for a loss whose TARGETS are not known when the stack's forward ends (stage-2 co-training,
 * train/loss.py:88-229: the agreement targets come from the EMA model): SWEEP_ONLY = the normalisations, the text launch and the statistics
 * sweep (none of them reads tgt / row_leak / g_v / g_t); FINISH_ONLY = the finishing launch (same-video blocks, positives, terms), after
 * a SWEEP_ONLY call on the same descriptor.  Neither flag: both, as before.  After FINISH_ONLY the last stage's same-video cosines
 * [B, T, N] f32 (padded-sentence order; what train/loss.py:280-283 takes its per-sentence maxima from) are at tan_simfam_diag(). */
#define TAN_SIMFAM_SWEEP_ONLY 4
#define TAN_SIMFAM_FINISH_ONLY 8
/* d_tn_acc is already ZERO when tan_simfam_bwd is called (the caller cleared it off the critical chain): the corrections launch does
 * not clear it (16 MB for the joint family at B = 128: 86 us in front of the one-pass kernel when it is the first thing after the
 * stage-2 step's meeting point) */
#define TAN_SIMFAM_ACC_ZEROED 16
typedef struct tan_simfam_desc {
    int S, St, B, T, N, C, Mc, flags;
    tan_ptr8 x_video; long v_grp_rows, v_off;
    tan_ptr8 x_text; long t_grp_rows, t_off;
    const long* idx; const int* colmap; const unsigned char* col_invalid;   /* [Mc] | [B*N] | [Mc] pad flags of the sweep's columns */
    const float* tgt; const unsigned char* row_leak;                        /* [B,T,N] f32 | [B*T] or NULL */
    void* vn; float* inv_v; void* tn; float* inv_t;
    float *rowsum, *colsum, *possum_v, *possum_t;
    void* e_keep; void* ws;
    float *v_terms, *t_terms;                                               /* out: [S,R], [S,Mc] */
    const float *g_v, *g_t;                                                 /* d loss / d terms: [S,R], [S,Mc] (fwd: optional) */
    void* dl; float* d_tn_acc;                                              /* bwd scratch: [S,R,Mc] bf16 + 256 elements of slack, [St,Mc,C] f32 */
    tan_ptr8 d_video; tan_ptr8 d_text;                                      /* out: stage-gradient rows (addressed like x_*) */
    int dtn_split_k;   /* K slices of the text-gradient GEMM; 0: default (St = 1: 8 slices of tan_gemm; St = S: 2 of tan_gemm_atb), < 0: -n slices of tan_gemm_atb */
} tan_simfam_desc;
long tan_simfam_ws_bytes(int S, int St, int B, int T, int N, int Mc);
/* != 0: the shape limits above hold (stages, N, Mc, the finishing launch's LDS bound): what both calls check of the dims before a launch */
int tan_simfam_accepts(int S, int St, int B, int T, int N, int Mc);
int tan_simfam_fwd(tan_simfam_desc* d, void* stream);
/* byte offset inside `ws` of stage s's same-video cosine blocks [B, T, N] f32 written by the finishing launch (every stage; entries of
 * padded sentences are their cosines without compaction and undefined with it: a dropped sentence has no sweep column) */
long tan_simfam_diag_offset(int S, int St, int B, int T, int N, int Mc, int s);
int tan_simfam_bwd(tan_simfam_desc* d, void* stream);

/* NCE tail (loss.py:236-237,254-275).  tan_pos_masks: rows_pos[b*T+t] = 1 if frame t of video b has a positive among its
 * unpadded sentences, cols_pos[b*N+k] = 1 if sentence k is unpadded and has a positive frame (tgt [B,T,N] f32, text_pad [B,N]).
 * tan_nce_tail_fwd: out2[0] = (mean(v_d | rows_mask) + mean(t_d | cols_mask)) / 2, out2[1] the same for the joint terms and
 * out2[2] = (out2[0] + out2[1]) / 2 (THREE floats; tan_nce_tail_bwd takes d loss / d each of them, any may be NULL = 0),
 * mean(x | m) = sum_{s,k} x[s,k] m[k] / (S sum m)  (NaN for an empty mask, like .mean() of nothing); counts2 = mask sums, kept
 * for tan_nce_tail_bwd, which turns d loss/d out2 into the gradients of the four term tensors.  One launch each.
 * counts_in (optional, [2]): divide by these (GLOBAL) mask sums instead of the local ones -- global negatives, row f3.     */
int tan_pos_masks(const float* tgt, const unsigned char* text_pad, float* rows_pos, float* cols_pos, int B, int T, int N, void* stream);
/* Stage-2 glue of get_loss (train/loss.py:280-290,309-328,345) in one launch, B*N <= 8192: from md / mj [B*N] (tan_diag_max of the dual /
 * joint last-stage same-video logits): metric = -(zscore(md) + zscore(mj)) over the real sentences, th = quantile(metric, q_th),
 * th_mask (bytes) / th_f = (metric <= th) & real, rows_pos_th [B*T] = rows that own a positive among the kept real sentences of tgt
 * [B,T,N]; with use_align: lab [B*N] (1 / 0 / 2 = ignore; 0 where the sentence's centre abs_text_pos.mean(-1) is < 0.2 or > 0.8;
 * NaN on padded sentences), sel = (lab != 2) & real, y = lab * sel; scal8 = {n_sel, n_pos, pos_weight = n_sel / n_pos - 1,
 * confidence ratio = mean(conf | real) (conf bytes or NULL), n_real, th, median(md), median(mj)}.
 * tan_bce_sel_fwd: out2 = {sum(BCEWithLogits(x, y, pos_weight) * sel) / n_sel, sum(((x > 0) == y) * sel) / n_sel};
 * tan_bce_sel_bwd: dx = g[0] * d bce / dx * sel / n_sel.                                                                           */
int tan_stage2_masks(const float* md, const float* mj, const unsigned char* text_pad, const float* tgt, const float* abs_text_pos,
                     const unsigned char* conf, float q_th, int use_align, int B, int T, int N, float* metric, unsigned char* th_mask,
                     float* th_f, float* rows_pos_th, float* lab, float* sel, float* y, float* scal8, void* stream);
int tan_bce_sel_fwd(const float* x, const float* y, const float* sel, const float* scal8, int n, float* out2, void* stream);
int tan_bce_sel_bwd(const float* x, const float* y, const float* sel, const float* scal8, const float* g, int n, float* dx, void* stream);
/* Everything get_loss derives from the batch's masks alone (train/loss.py:58-70: pad masks, the [B,T,N] start/end target) in one launch,
 * plus the text-column compaction of the logits-free sweeps: text_pad as f32 0/1 (train/main.py:62-65) OR as bytes (exactly one non-NULL),
 * video_pad bytes [B,T], tgt_raw bytes [B,N,T] (get_mask_from_time) -> tpad_u8 / valid (bytes) / valid_f (f32) [B*N], vpad_u8 [B*T],
 * tgt f32 [B,T,N]; with idx != NULL also idx [Mc] (int64: real sentences in order, then padded columns in order = a stable sort of the
 * pad flags), colmap [B*N] (int32 rank among the real sentences, -1 = padded), ci_run [Mc] (pad flags of the compacted columns).      */
int tan_loss_prep(const float* text_pad_f32, const unsigned char* text_pad_u8, const unsigned char* video_pad_u8,
                  const unsigned char* tgt_raw, unsigned char* tpad_u8, unsigned char* vpad_u8, unsigned char* valid, float* valid_f,
                  float* tgt, long* idx, int* colmap, unsigned char* ci_run, int B, int T, int N, int Mc, void* stream);
int tan_nce_tail_fwd(const float* v_d, const float* t_d, const float* v_j, const float* t_j, const float* rows_mask,
                     const float* cols_mask, int Sd, int Sj, long R, long M, float* out2, float* counts2, const float* counts_in,
                     void* stream);
int tan_nce_tail_bwd(const float* g_dual, const float* g_joint, const float* g_mean, const float* rows_mask, const float* cols_mask,
                     const float* counts2, int Sd, int Sj, long R, long M, float* g_v_d, float* g_t_d, float* g_v_j, float* g_t_j,
                     void* stream);

/* ---- sentence embedder (model/word2vec_model.py:76-102) ----------------------------------------
 * tan_embed_gather: out[r, 0:D] = table[ids[r], :] cast to `dtype`, out[r, D:Dpad] = 0 (ids NULL = identity: a padded
 *   cast of a [rows, D] f32 matrix).  Pads the 300-d word vectors / fc1 weight rows to a multiple of 64 for the MFMA GEMM.
 * tan_unpad_add: dst[r, 0:D] += src[r, 0:D] for src [rows, Dpad] f32 (the padded dW1 back into the 300-wide gradient).
 * tan_wordpool_fwd: pooled[m,j] = max_w (mask[m,w] ? h[m,w,j] : -6e4), argmax[m,j] = first maximising w
 *   (masked_fill + torch.max, word2vec_model.py:94-96); tan_wordpool_bwd: dh[m,w,j] = (w == argmax && pooled > 0) ? d_pooled : 0,
 *   i.e. the max routing followed by the in-place ReLU's gradient; db1 (optional, f32 [H]) += column sums of dh.            */
int tan_embed_gather(const long* ids, const float* table, void* out, long rows, int D, int Dpad, long V, int dtype, void* stream);
int tan_unpad_add(const float* src, float* dst, long rows, int D, int Dpad, void* stream);
int tan_wordpool_fwd(const void* h, const unsigned char* mask, void* pooled, int* argmax, long M, int W, int H, int dtype,
                     void* stream);
int tan_wordpool_bwd(const void* d_pooled, const void* pooled, const int* argmax, void* dh, float* db, long M, int W, int H,
                     int dtype, void* stream);

/* ---- fused AdamW (+ EMA twin, + bf16 shadow weights) over one flat f32 parameter buffer ---------------------
 * torch.optim.AdamW single-tensor arithmetic (train/main.py:397, groups of main.py:330-356) followed by
 * TwinTemporalAligner._momentum_update (tan_model.py:339-344).  mode[i]: 0 no decay, 1 decay, 2 parameter never
 * receives a gradient (skipped like a .grad-is-None parameter), 3 frozen for the optimizer, still EMA'd; NULL = all decay.
 * Modes 2 and 3 leave p, m, v and p_bf16 untouched; the EMA twin (ema, ema_bf16) moves from the unchanged p in every mode.
 * step >= 1 is the 1-based count. */
int tan_adamw_step(float* p, const float* g, float* m, float* v, const unsigned char* mode, long n, double lr,
                   double beta1, double beta2, double eps, double weight_decay, int step, float grad_scale, void* p_bf16,
                   float* ema, float ema_m, void* ema_bf16, void* stream);
/* tan_adamw_step plus every weight IMAGE the bf16 kernels read, in the same pass: for each [N][K] matrix of `table` (DEVICE memory;
 * off = element offset in the flat buffers, shared by all images) the updated values are also written as the row-major W^T (p_t), the
 * tan_pack_weights image of W in tiles [tn_w][tk_w] (p_packed; tn_w = 384 selects "qkv16", 0 = none) and of W^T in tiles [tn_t][tk_t]
 * (p_tpacked), and the EMA twin's packed W (ema_packed); any image pointer may be NULL.  unit_prefix (DEVICE, [n_entries + 1]) =
 * running sum of N/64 * K/64 over the table, n_units its last element; N % 64 == 0, K % 64 == 0.  mode (required) as in
 * tan_adamw_step, but read ONCE per matrix, at mode[off]: a table matrix must carry a uniform mode (a matrix in mode 2 or 3 keeps
 * p, m, v and still gets every image rewritten from its current values); rest_idx (DEVICE, int32 [n_rest], ascending) lists every element of the flat buffer OUTSIDE the table's matrices:
 * those are updated by the plain kernel in a second launch.  Replaces tan_adamw_step + tan_transpose_batch + 2 x tan_pack_weights of a training step (train/main.py:112-122). */
typedef struct tan_image_entry { long off; int N, K, tn_w, tk_w, tn_t, tk_t; } tan_image_entry;
typedef struct tan_adamw_images_desc {
    float* p; const float* g; float *m, *v; const unsigned char* mode; long n;
    double lr, beta1, beta2, eps, weight_decay; int step; float grad_scale;
    void* p_bf16; float* ema; float ema_m; void* ema_bf16;
    const tan_image_entry* table; const long* unit_prefix; int n_entries; long n_units;
    void *p_packed, *p_t, *p_tpacked, *ema_packed;
    const int* rest_idx; long n_rest;
    long unit_begin, unit_end;   /* only the table's units [unit_begin, unit_end) (unit_end == 0: to n_units): a step may update the matrices whose
                                    gradients are final early -- e.g. one stack's while the other's backward still runs -- and the rest,
                                    with rest_idx, in a second call */
} tan_adamw_images_desc;
int tan_adamw_step_images(const tan_adamw_images_desc* d, void* stream);
/* target = m*target + (1-m)*online  (TwinTemporalAligner._momentum_update, tan_model.py:339-344) */
int tan_ema_update(float* target, const float* online, long n, float m, void* target_bf16, void* stream);

/* ---- per-parameter gradient clipping over the flat f32 gradient buffer (utils/train_utils.py:3-13, called at train/main.py:115-116) ----
 * Every parameter tensor is a SEGMENT of g [n] (n < 2^31), cut into chunks of at most tan_clip_chunk() elements.  chunk_table (DEVICE,
 * int32 [n_chunks][4], 16-byte aligned) = (off, len, seg, 0) per chunk; seg_table (DEVICE, int32 [n_segs][2]) = (first_chunk, n_chunks)
 * per segment, a segment's chunks consecutive.  Both calls work on the chunks [c0, c1) and the segments [s0, s1), which must hold
 * exactly those chunks (a caller orders the tables so that one range is one group of parameters); one workgroup per chunk, no atomics:
 * the same input gives the same bits whatever the scheduling.  A table entry outside [0, n), or a segment that is not wholly inside
 * the ranges, is skipped.
 *   tan_clip_sumsq   partials[chunk] = the chunk's sum of squares (f32: per-thread accumulators, wave tree, four waves through LDS).
 *   tan_clip_apply   per segment: norm = sqrt(sum of its partials, in table order, in double) * grad_scale, coef = clip / (norm + 1e-6f);
 *                    g[segment] *= coef if coef < 1, otherwise nothing is stored (a NaN norm leaves the segment as it is, like the
 *                    reference's `if clip_coef < 1`); norms[seg] = norm.  g keeps the UNSCALED gradient: grad_scale (1 / world size) is
 *                    what tan_adamw_step applies afterwards, so norm is the norm of the gradient the optimizer sees.
 * Elements between segments (alignment padding) are never read or written. */
int tan_clip_chunk(void);
int tan_clip_sumsq(const float* g, const int* chunk_table, const int* seg_table, int c0, int c1, int s0, int s1, long n,
                   float* partials, void* stream);
int tan_clip_apply(float* g, const int* chunk_table, const int* seg_table, int c0, int c1, int s0, int s1, long n,
                   const float* partials, float clip, float grad_scale, float* norms, void* stream);

/* ---- one TemporalEncoder stack (tfm_model.py:41-55), forward and backward in one call each -----------------
 * Weights are `dtype` (f32, or the bf16 shadow copies); biases / LayerNorm affine / all gradients are f32 and
 * gradients are ACCUMULATED.  Layouts: w_qkv [3C,C] (in_proj_weight, q|k|v), w_out [C,C], w_fc [4C,C], w_proj [C,4C]. */
typedef struct tan_layer_params {
    const void *w_qkv, *w_out, *w_fc, *w_proj;
    const float *b_qkv, *b_out, *b_fc, *b_proj;
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    float *g_w_qkv, *g_w_out, *g_w_fc, *g_w_proj;
    float *g_b_qkv, *g_b_out, *g_b_fc, *g_b_proj;
    float *g_ln1_g, *g_ln1_b, *g_ln2_g, *g_ln2_b;
    const void *wt_qkv, *wt_out, *wt_fc, *wt_proj; /* optional (bf16): W^T copies, [in, out] row-major, for the dX GEMMs; NULL = read W K-strided */
    const void *wp_qkv, *wp_out, *wp_fc, *wp_proj; /* optional (bf16): tan_pack_weights images of w_* for the row-panel kernels; NULL = unfused path */
    const void *wtp_qkv, *wtp_out, *wtp_fc, *wtp_proj; /* optional (bf16): tan_pack_weights images of wt_* (backward row-panel kernels) */
} tan_layer_params;

/* per-layer saved activations, rows R = B*L */
typedef struct tan_layer_bufs {
    void *xn1, *qkv, *attn_o, *x_mid, *xn2, *h_pre, *h_act, *x_out; /* dtype: [R,C] [R,3C] [R,C] [R,C] [R,C] [R,4C] [R,4C] [R,C] */
    float *mean1, *rstd1, *mean2, *rstd2;                            /* [R] */
    float* lse;                                                      /* [B,H,L] */
} tan_layer_bufs;

typedef struct tan_encoder_desc {
    int dtype, B, L, C, H, layers;
    const unsigned char* key_padding_mask; /* [B,L] bytes, 1 = ignore, or NULL */
    const void* x0;                        /* [R,C] stack input */
    const tan_layer_params* params;        /* HOST array [layers] of device pointers */
    const tan_layer_bufs* bufs;            /* HOST array [layers] */
    const float *post_g, *post_b;          /* ln_video_post_enc / ln_joint_post_enc (tan_model.py:174,206) */
    float *g_post_g, *g_post_b;
    void* post_out;                        /* [R,C] last stage = LN_post(x_out[last]); NULL to skip */
    float *post_mean, *post_rstd;
    /* backward only */
    void *scr_dx, *scr_dx2, *scr_do, *scr_dxn; /* [R,C] */
    void* scr_dh;                               /* [R,4C] */
    void* scr_dqkv;                             /* [R,3C] */
    float* ln_ws;                               /* tan_layernorm_bwd_ws_floats(C) */
    float* dw_ws;                               /* split-K partial tiles for the dW GEMMs, or NULL (then f32 atomics) */
    long dw_ws_floats;                          /* >= 32 * 4*C*C to cover every layer shape */
    const void* const* d_stage;                 /* HOST array [layers]: grad w.r.t. stage s ([R,C] dtype) or NULL */
    void* d_x0;                                 /* [R,C] out: grad w.r.t. x0 */
    void* const* layer_done;                    /* HOST array [layers] of tan_event handles or NULL: layer_done[i] is recorded on
                                                   the stream once every gradient of layer i's parameters is final (layers finish
                                                   last to first) -- lets a data-parallel caller start reducing a layer's slice of
                                                   the flat gradient while the earlier layers' backward still runs.  Not together
                                                   with an effective dw_tail > 0 (dw_stream set and not the stack's stream): the tail
                                                   blocks' weight gradients are not final on the stream, so tan_encoder_bwd returns -1 */
    /* forward only */
    int no_save;                                /* != 0: no backward will follow (torch.no_grad(): the EMA target's forward,
                                                   tan_model.py:348-351, and every evaluation entry point) -- the tensors that exist
                                                   only for backward (h_pre, h_act, xn2, mean2 / rstd2, and on the fused attention
                                                   path qkv, attn_o, lse) are NOT written; bufs[] may then leave them NULL.  The stage
                                                   outputs (xn1 of layers >= 1, post_out) and x_mid / x_out are written as usual. */
    /* forward only: != 0: bufs[0].xn1 / mean1 / rstd1 already hold the first block's ln_1(x0) (tan_embed_fwd wrote them) */
    int xn1_ready;
    /* backward only, optional: the grouped weight-gradient launches of blocks dw_tail - 1 .. 0 -- the LAST blocks of a stack's backward;
     * they only feed the optimizer -- go to dw_stream (made to wait for the stack's stream first), so that the stack's remaining dX kernels
     * and whatever the caller queues behind tan_encoder_bwd (the embeddings' backward) do not wait for them.  Block 0 needs nothing else
     * (nothing overwrites its operands any more); dw_tail > 1 needs the second set of the four scratch buffers such a launch reads
     * (scr2_*): the tail blocks alternate between the sets, and a block waits for the launch two blocks above it before it reuses
     * a set.  The CALLER joins dw_stream before it reads those weight gradients or reuses the scratch buffers. */
    void* dw_stream; int dw_tail;
    void *scr2_dx, *scr2_dx2, *scr2_dh, *scr2_dqkv;
    /* optional, both directions: scratch [8, R, C] f32 -- with it, stacks of few row panels (R / 64 <= TAN_SPLIT_PANELS, default 48)
     * run the MLP branch through tan_mlp_fwd_split / tan_mlp_bwd_split */
    float* split_part;
    /* forward only, optional: the forward in TWO VIDEO GROUPS.  The stack's forward is row-local per video (one attention workgroup per
     * video, one MLP workgroup per 64-row panel, the LayerNorms inside both), so videos [0, fwd_group_videos) run the whole layer loop
     * on the call's stream and videos [fwd_group_videos, B) the same launches -- every per-row / per-video pointer advanced, B and the
     * row count reduced -- on fwd_group_stream, which is made to wait for the call's stream first and which the call's stream waits for
     * before tan_encoder_fwd returns: everything is ordered on the call's stream as without groups, and every result is bit-identical.
     * Two half-size launch chains per stack instead of one: when a launch ends, another chain's next launch takes the CUs (DESIGN.md
     * section 3.7).  Taken only where the whole-panel launches run (bf16, C = 512, the fused attention branch's L, images bound, not
     * the split-hidden path), 0 < fwd_group_videos < B and both groups' rows are multiples of 64; anything else -- NULL / 0 included
     * -- is the ungrouped forward, launch for launch. */
    void* fwd_group_stream; int fwd_group_videos;
} tan_encoder_desc;
int tan_encoder_fwd(const tan_encoder_desc* e, void* stream);
int tan_encoder_bwd(const tan_encoder_desc* e, void* stream);

/* Weight gradient of a Linear layer (what autograd produces for nn.Linear.weight inside model/tfm_model.py's blocks):
 * gw[N,K] (f32) += dy[M,N]^T x[M,K].  The long M contraction is cut into slices; with a workspace `ws` (>= slices*N*K floats,
 * slices <= 32) they are written as partial tiles and folded by tan_reduce_add, otherwise accumulated with f32 atomics. */
int tan_linear_wgrad(const void* dy, const void* x, float* gw, long M, int N, int K, float* ws, long ws_floats, int dtype,
                     void* stream);
/* C_p [M_p, N_p] (=|+=) A_p^T B_p for p < n <= 8 problems sharing the contraction length K (a multiple of 128): A_p [K, lda_p] and
 * B_p [K, N_p] row-major bf16 -- the contraction runs over ROWS.  256 x 256 tiles (N_p % 256 == 0; M_p ragged: the last tile of A_p's
 * columns reads up to 255 elements past each row, so the caller pads the END of A_p's buffer by 512 bytes).  out_dtype TAN_BF16: plain
 * store (split == 1, accumulate == 0); TAN_F32: split == 1 stores or (accumulate) adds in place, split > 1 K slices add with f32
 * atomics (accumulate must be set; C zeroed by the caller).  This is the kernel behind tan_linear_wgrad_group (the weight gradients
 * dW = dY^T X of a block, autograd of model/tfm_model.py:21-27) with its full shape range exposed. */
int tan_gemm_atb(int n, const void* const* A, const void* const* B, void* const* C, const int* lda, const int* M, const int* N, long K,
                 int out_dtype, int accumulate, int split, void* stream);
/* The weight gradients of up to four Linear layers over the same M rows (the in_proj, out_proj, c_fc and c_proj of one
 * ResidualAttentionBlock, tfm_model.py:17-27) in ONE launch: gw[i][N[i],K[i]] += dy[i][M,N[i]]^T x[i][M,K[i]].  This is the call
 * tan_encoder_bwd makes per block; not eligible groups (f32, ragged M) run tan_linear_wgrad one by one.               */
int tan_linear_wgrad_group(int n, const void* const* dy, const void* const* x, float* const* gw, const int* N, const int* K,
                           long M, float* ws, long ws_floats, int dtype, void* stream);

/* ---- row-panel fused kernels: one launch per half block ("fused layer") ------------------------
 * A workgroup owns a 64-row panel of the residual stream and keeps it in LDS while the weights stream past it from L2; the
 * weights are PRE-PACKED (once per optimizer step) into the LDS image of the tiles the kernels consume, in consumption order.
 * tan_pack_weights: entry i packs the row-major bf16 matrix src[src_off ..] of shape [N][K] (the nn.Linear layout, or a W^T
 *   copy) into dst[dst_off ..] as tiles [TN][TK] in (n-block, k-block) order; TN*TK*2 bytes must be 16384, TK in {16,32,64}
 *   (kernels here: TN=256,TK=32 for N > 512, TN=512,TK=16 for N == 512; TN=384,TK=32 with N=1536 selects the "qkv16" format of
 *   tan_attnblk_fwd: 24-KiB tiles of 16 x 32 fragments, see there).  `table` is DEVICE memory; max_tiles = the largest
 *   N/TN * K/TK of the table. */
typedef struct tan_pack_entry { long src_off, dst_off; int N, K, TN, TK; } tan_pack_entry;
int tan_panel_waves(void);   /* waves per row-panel workgroup the library was built for (fragment ownership inside a packed tile) */
int tan_pack_weights(const void* src, void* dst, const tan_pack_entry* table, int n, int max_tiles, void* stream);

/* tan_mlp_fwd: the MLP half of ResidualAttentionBlock_Step.forward (model/tfm_model.py:23-27,37) for rows % 64 == 0, bf16:
 *   xn2 = LN2(x_mid) ; h = QuickGELU(xn2 W_fc^T + b_fc) ; x_out = x_mid + h W_proj^T + b_proj ; xn_next = LN_next(x_out)
 * xn2 / mean2 / rstd2 / h_pre / h_act are saved for backward (each group may be NULL: not stored -- h_pre and h_act together,
 * mean2 and rstd2 together, xn2 alone; the no-grad forward passes none of them); xn_next (optional) is the
 * NEXT block's ln_1 output (= this block's deep-supervision feature, tfm_model.py:48-55) or the stack's post-LN.
 * pw_fc = packed c_fc.weight [2048][512] (TN=256,TK=32), pw_proj = packed c_proj.weight [512][2048] (TN=512,TK=16).      */
typedef struct tan_mlp_desc {
    long rows; int C, FF;                    /* 512, 2048 */
    const void* x_mid;                       /* [rows, C] bf16 */
    const float *ln_g, *ln_b;                /* ln_2 */
    const void *pw_fc, *pw_proj;
    const float *b_fc, *b_proj;
    void* xn2; float *mean2, *rstd2;         /* out */
    void *h_pre, *h_act;                     /* out [rows, FF] bf16 or NULL */
    void* x_out;                             /* out [rows, C] */
    const float *nln_g, *nln_b;              /* optional fused LayerNorm of x_out */
    void* xn_next; float *nmean, *nrstd;
    float eps;
    int variant;                             /* 0; (1: stream only, 2: no streaming -- timing experiments, results undefined) */
    /* Optional head (pw_out != NULL): x_mid is not read but WRITTEN first, x_mid = x_in + attn_o W_out^T + b_out -- the attention
     * out-projection + bias + residual of the block (tfm_model.py:30-36: what follows the attention core) for shapes the one-launch
     * attention branch (tan_attnblk_fwd) does not take (L > 80): attn_o [rows, C] bf16 = tan_attn_fwd's output, pw_out =
     * tan_pack_weights image of out_proj.weight [C][C] (TN = 512, TK = 16), b_out f32 [C], x_in [rows, C] bf16 the block's input. */
    const void* attn_o; const void* pw_out; const float* b_out; const void* x_in;
} tan_mlp_desc;
int tan_mlp_fwd(const tan_mlp_desc* d, void* stream);

/* Backward of the same branch in ONE launch (replaces, in tan_encoder_bwd: the c_proj dX GEMM with its quickgelu' epilogue and
 * bias column sums, the c_fc dX GEMM, and the ln_2 backward kernel; reference: autograd of model/tfm_model.py:23-27,37,44):
 *   dh  = (dx W_proj) o quickgelu'(h_pre)                  -> dh [rows, FF] bf16 (operand of the c_fc weight gradient)
 *   dx2 = dx + LayerNorm-backward(dh W_fc; x_mid, mean2, rstd2, ln_g)      -> dx2 [rows, C] bf16
 *   g_b_fc += colsum(dh), g_ln_g += colsum(dxn o xhat), g_ln_b += colsum(dxn), g_b_out += colsum(dx2)     (f32 atomics)
 * pwt_proj = tan_pack_weights image of W_proj^T [2048][512] (TN=256,TK=32), pwt_fc = of W_fc^T [512][2048] (TN=512,TK=16).
 * rows % 64 == 0, C = 512, FF = 2048, bf16 only.                                                                             */
typedef struct tan_mlp_bwd_desc {
    long rows; int C, FF;
    const void* dx;                          /* [rows, C] gradient w.r.t. the block's output (also the residual gradient); see ln1_dxn */
    const void* h_pre;                       /* [rows, FF] pre-activation saved by the forward */
    const void* x_mid;                       /* [rows, C] the branch's input (ln_2 input) */
    const float *mean2, *rstd2, *ln_g;
    const void *pwt_proj, *pwt_fc;
    void* dh;                                /* out [rows, FF] */
    void* dx2;                               /* out [rows, C] */
    float *g_b_fc, *g_ln_g, *g_ln_b, *g_b_out;   /* accumulated */
    /* Optional (ln1_dxn != NULL): `dx` is not read but PRODUCED first, as the backward of the NEXT block's ln_1 (tfm_model.py:43):
     *   dx = ln1_res + LayerNorm-backward(ln1_dxn; ln1_x, ln1_mean, ln1_rstd, ln1_g)      -> dx_out [rows, C] bf16 (and the panel)
     *   g_ln1_g += colsum(ln1_dxn o xhat), g_ln1_b += colsum(ln1_dxn), g_dx_colsum += colsum(dx)  (= this block's c_proj bias grad)
     * ln1_res may alias dx2 (a workgroup reads its 64 rows before it writes them) or be NULL (no residual: the stack's post-LayerNorm). */
    const void *ln1_dxn, *ln1_x, *ln1_res;
    const float *ln1_mean, *ln1_rstd, *ln1_g;
    float *g_ln1_g, *g_ln1_b, *g_dx_colsum;
    void* dx_out;
    /* Optional tail (pwt_out != NULL): d_o [rows, C] bf16 = dx2 W_out -- the dX GEMM of the block's attention out-projection
     * (tfm_model.py:21: attn.out_proj), whose input gradient dx2 is sitting in this kernel's LDS panel; pwt_out = tan_pack_weights
     * image of out_proj.weight^T with TN = 512, TK = 16.  Saves the 8192 x 512 x 512 launch of tan_encoder_bwd. */
    const void* pwt_out;
    void* d_o;
    /* Optional head (pwt_in != NULL; needs the ln_1 fields above, ln1_dxn = NULL): ln1_dxn is PRODUCED first, in LDS only:
     *   ln1_dxn = dqkv W_in (+ dstage)  -- the dX GEMM of the NEXT block's attention in-projection (tfm_model.py:21: attn.in_proj) with
     * dqkv [rows, 3C] bf16 (tan_attn_bwd's output), pwt_in = tan_pack_weights image of in_proj_weight^T [C][3C] (TN = 512, TK = 16),
     * dstage [rows, C] bf16 or NULL = the deep-supervision gradient that joins at that ln_1 output.  Saves the 8192 x 1536 x 512
     * launch per block of tan_encoder_bwd and the [rows, C] round trip of its result. */
    const void* dqkv;
    const void* pwt_in;
    const void* dstage;
} tan_mlp_bwd_desc;
int tan_mlp_bwd(const tan_mlp_bwd_desc* d, void* stream);

/* Small batches (round 6): the same two branches with the HIDDEN dimension split over tan_mlp_split_chunks() = 8 workgroups per 64-row
 * panel.  A whole-panel workgroup streams all of its block's weights (4 MiB) whatever the batch, so 16 panels take as long as 160; here
 * workgroup (panel, chunk) runs one 256-wide hidden chunk (the same prologue, c_fc / c_proj phases, chunk epilogue and side outputs) and
 * stores its [64 x 512] f32 term as plane `chunk` of `part` [8, rows, C] (scratch: nothing is expected in it, nothing is left in it
 * that matters); a second launch adds the eight planes in chunk order and applies the row epilogue -- forward: + b_proj + residual ->
 * x_out and the optional next LayerNorm (tfm_model.py:37,43); backward: LayerNorm-2 backward + residual -> dx2 and the column-sum
 * parameter gradients.  Same descriptors and results (to the order of eight f32 additions) as tan_mlp_fwd / tan_mlp_bwd; the optional
 * head / tail / ln_1-prologue fields must be NULL (tan_encoder_* issues those pieces as the launches they were before they were folded
 * in).                                                                                                                               */
int tan_mlp_split_chunks(void);
int tan_mlp_fwd_split(const tan_mlp_desc* d, float* part, void* stream);
int tan_mlp_bwd_split(const tan_mlp_bwd_desc* d, float* part, void* stream);

/* ---- input embeddings in ONE launch (bf16 throughput mode, C = 512) ------------------------------------------------------------
 * tan_embed_fwd: per problem (modality), rows r = (video v, position t) with t = r % T:
 *   proj = a W^T;  y = LayerNorm(proj; ln_g, ln_b);  out[d][(v*out_grp_rows[d] + out_off[d] + t)] = y + pos[d][t]   (d = 0, 1)
 *   xn1[d] = LayerNorm(out[d]; ln1_g[d], ln1_b[d])  with mean1 / rstd1 at the same row index        (optional)
 * replaces model/tan_model.py:155-167 + 187-203 (video_pre_proj, ln_video_init, ln_position_init(pos[p0:p0+T]) for the dual and the
 * joint offset, the torch.cat into the joint stack's input) resp. 231-234 / 212-228 (text) and the first block's ln_1 of the stack
 * that consumes out[d] (model/tfm_model.py:35).  a: [rows, K] f32 or bf16 (a_dtype); pw: tan_pack_weights image of W [512][K] with
 * TN = 512, TK = 16; pos[d]: f32 [T, 512] rows ALREADY normalised by ln_position_init (or NULL); a_bf16 (optional, when a is f32):
 * the bf16 copy of a the weight-gradient GEMM of the backward reads; proj / mean / rstd: saved for the LayerNorm backward.
 * pad_dst (optional): pad_dst[v*pad_grp_rows + pad_off + t] = pad_src[r] (or 0): the rows' key-padding flags in the joint [B, L] mask.
 * Up to two problems (video, text) share one launch. */
typedef struct tan_embed_desc {
    const void* a; int a_dtype; long rows; int K, T, C;
    const void* pw; const float *ln_g, *ln_b;
    void* a_bf16; void* proj; float *mean, *rstd;
    void* out[2]; long out_grp_rows[2], out_off[2]; const float* pos[2];
    const float *ln1_g[2], *ln1_b[2]; void* xn1[2]; float *mean1[2], *rstd1[2];
    const unsigned char* pad_src; unsigned char* pad_dst; long pad_grp_rows, pad_off;
} tan_embed_desc;
int tan_embed_fwd(const tan_embed_desc* d, int nprob, void* stream);

/* tan_embed_bwd: backward of tan_embed_fwd's LayerNorm + position add for up to two problems in one launch (autograd of
 * model/tan_model.py:155-167, 187-199, 212-234): dy = d_out[0] + d_out[1] (either may be NULL; rows addressed like tan_embed_fwd's out[]:
 *   row v*d_out_grp_rows[d] + d_out_off[d] + t, and a present d_out[d] needs 0 <= d_out_off[d] and T + d_out_off[d] <= d_out_grp_rows[d]),
 *   d_proj [rows, C] bf16 = LayerNorm-backward(dy; proj, mean, rstd, ln_g)   (operand of the pre-projection's weight gradient)
 *   g_ln_g += colsum(dy o xhat), g_ln_b += colsum(dy);  d_pos[d] [ceil(videos / tan_embed_bwd_group())][T, C] f32 = per video GROUP,
 *   the sum over its videos of d_out[d] (plain stores, every plane written in full; NULL = not wanted; tan_pos_ln_bwd adds the planes)
 * tan_pos_ln_bwd: ln_position_init's backward for up to three used table slices in one launch: g_table rows += LayerNorm-backward(sum of
 *   the nparts planes d_pos [nparts][n][C];
 *   x = the raw table rows, mean, rstd, gamma) (g_table NULL: a fixed sine table), g_gamma += colsum(d_pos o xhat), g_beta += colsum(d_pos);
 *   f32 atomics (the slices of the dual and the joint offset overlap). */
typedef struct tan_embed_bwd_desc {
    long rows; int T, C;
    const void* d_out[2]; long d_out_grp_rows[2], d_out_off[2];
    const void* proj; const float *mean, *rstd, *ln_g;
    void* d_proj; float *g_ln_g, *g_ln_b; float* d_pos[2];
} tan_embed_bwd_desc;
int tan_embed_bwd(const tan_embed_bwd_desc* d, int nprob, void* stream);
typedef struct tan_pos_ln_bwd_use { const float *d_pos, *x, *mean, *rstd; float* g_table; int n, nparts; } tan_pos_ln_bwd_use;
int tan_embed_bwd_group(void);   /* videos per partial plane of tan_embed_bwd's d_pos */
int tan_pos_ln_bwd(const tan_pos_ln_bwd_use* u, int nuse, const float* gamma, float* g_gamma, float* g_beta, int C, void* stream);

/* ---- the attention branch of a block in ONE launch per direction (bf16, C = 512, H = 8, 48 < L <= 80 rows per video) --------
 * tan_attnblk_fwd: x_mid = x_in + out_proj(MHA(xn1))  with MHA = nn.MultiheadAttention(512, 8) as called at
 * model/tfm_model.py:30-36 (packed in_proj q|k|v, q scaled by 64^-0.5, key_padding_mask keys = -inf, softmax over keys, dropout 0,
 * need_weights=False).  One workgroup per video keeps the xn1 panel in LDS; replaces the in_proj GEMM, tan_attn_fwd and the
 * out_proj GEMM (+bias +residual) of tan_encoder_fwd, and the qkv / attn_o round trips between them.
 *   pw_qkv = tan_pack_weights image of attn.in_proj_weight [1536][512] with TN = 384, TK = 32 (the "qkv16" format: tile (head
 *            pair hp, k step) holds, per wave w and feature block fb < 3, the 16 x 32 fragment of in_proj rows
 *            which*512 + (2hp + j)*64 + fblk*16 .. +15 where p = 3w + fb, which = (p / 4) % 3, j = p / 12, fblk = p % 4)
 *   pw_out = tan_pack_weights image of attn.out_proj.weight [512][512] with TN = 512, TK = 16
 * qkv [B*L, 3C], attn_o [B*L, C], lse [B, H, L] are what tan_attn_bwd needs later: all three or none (NULL: the no-grad forward
 * writes nothing but x_mid).  Fully padded key rows give zeros (lse = -inf), like tan_attn_fwd.                              */
typedef struct tan_attnblk_desc {
    int B, L, C, H;
    const void* xn1;                         /* [B*L, C] bf16: ln_1 output */
    const void* x_in;                        /* [B*L, C] bf16: the residual stream entering the block */
    const unsigned char* key_padding_mask;   /* [B, L] bytes, 1 = ignore, or NULL */
    const void *pw_qkv, *pw_out;
    const float *b_qkv, *b_out;
    void *qkv, *attn_o; float* lse;          /* out, saved for backward, or all NULL */
    void* x_mid;                             /* out [B*L, C] */
} tan_attnblk_desc;
int tan_attnblk_supported(int L, int C, int H, int dtype);
int tan_attnblk_fwd(const tan_attnblk_desc* d, void* stream);
/* Small batches (round 6): the same branch with one workgroup per (video, head pair) -- B workgroups leave most of the chip idle for
 * 50-70 us per launch at B = 16 -- each storing its [L x 512] f32 term of the out-projection as plane `hp` of `part` (scratch
 * [4, B*L, C] f32); a second launch adds the four planes in order, + b_out + x_in -> x_mid.  Same descriptor, same side outputs. */
int tan_attnblk_fwd_split(const tan_attnblk_desc* d, float* part, void* stream);

/* tools/lab only: device buffer ([8 waves][64] long) that receives workgroup 0's shader clock at the phase boundaries of
 * tan_attnblk_fwd, or NULL (default): no instrumentation */
int tan_attnblk_lab_set_dbg(void* device_buffer);

/* ---- corpus auto-alignment (HTM-AA inference; the evaluation loop of eval/eval_zeroshot_align.py:129-223 over MANY videos) ----
 * Videos, sentences and windows of a chunk are packed: video features [sum vlen, Dv], sentence embeddings [sum K, Dt], and an
 * int32 window table of TAN_WIN_FIELDS per window, in plan order (videos in chunk order, windows by start time):
 *   vrow (packed frame row of s0), t (= e0 - s0), krow (packed sentence row of the first active sentence), k (active sentences),
 *   s0, vlen, aoff (the video's first element in the [K, vlen] accumulators), kbase (packed row of the video's sentence 0).
 * A pass is a contiguous slice of the table (W windows, pointer offset by the caller).                                         */
#define TAN_WIN_FIELDS 8
/* One pass's model input in one launch: out_video [W, T, Dv] (frames beyond t zero), out_vmask [W, T] bytes (1 = padding),
 * out_text [W, Kp, Dt] (rows beyond k zero), out_tmask [W, Kp] -- the slicing of train/main.py:171-189's per-window calls,
 * stacked.  A bit copy: *_elem_bytes = 2 (f16 / bf16) or 4 (f32), the outputs have the inputs' element type.                   */
int tan_window_pack(const void* video, int video_elem_bytes, int Dv, const void* text, int text_elem_bytes, int Dt,
                    const int* table, int W, int T, int Kp, void* out_video, unsigned char* out_vmask, void* out_text,
                    unsigned char* out_tmask, void* stream);
/* acc_j / acc_d [sum K*vlen] += the pass's last-stage joint / dual similarities x (1/0.07) (eval_zeroshot_align.py:197-201),
 * cnt += 1 over each window's [k, t] block; tcnt [sum K] += 1 per window holding the sentence and, with the alignability head
 * (a_joint = the joint stage-2 head logits [W, Kp], eval_zeroshot_align.py:186), a_sum [sum K] += them.  sim_j / sim_d: one
 * stage of eval_windows' output, [W, T, Kp] f32.  Each element adds its windows in window order (no atomics): f32-identical to
 * the host loop, however the windows are cut into passes.  a_joint and a_sum are both NULL without the head.                    */
int tan_window_stitch_acc(const float* sim_j, const float* sim_d, const float* a_joint, const int* table, int W, int T, int Kp,
                          float* acc_j, float* acc_d, float* cnt, long n_acc, float* tcnt, float* a_sum, long n_rows,
                          void* stream);
/* Per sentence row g (rows [n_rows, 2] int32 = accumulator offset, vlen): acc_j row <- sim = (acc_j/max(cnt,1e-5) +
 * acc_d/max(cnt,1e-5)) / 2, 0 -> -6e4 (eval_zeroshot_align.py:199-205,221); res [4, n_rows] f32 = first arg-max of the row,
 * max of its softmax over time, score (a_sum / max(tcnt, 1e-5) with the head, else the row max, :219-223), tcnt > 0.          */
int tan_window_stitch_final(float* acc_j, const float* acc_d, const float* cnt, const float* tcnt, const float* a_sum,
                            const int* rows, long n_rows, long n_acc, float* res, void* stream);
/* Order-preserving timestamps: a monotonic decode over the stitched rows, in place of the independent per-row arg-max of
 * eval_zeroshot_align.py:222,237 (ASR sentences are spoken in order; nothing in an arg-max per row respects that).  Per video, with
 * its kept rows r_0 .. r_{m-1} in decode order, V = vlen and x_i[t] = sim[r_i][t] (the f32 rows tan_window_stitch_final leaves,
 * -6e4 cells included, used as they are):
 *     D_0[t] = x_0[t];   D_i[t] = x_i[t] + M_{i-1}[t]   -- one f32 add, round to nearest, never contracted
 *     M_i[t] = max_{t' <= t} D_i[t'];   A_i[t] = the SMALLEST t' <= t with D_i[t'] == M_i[t]
 *     t_{m-1} = A_{m-1}[V-1];   t_{i-1} = A_{i-1}[t_i];   path score = D_{m-1}[t_{m-1}]
 * The seconds are non-decreasing (equal seconds allowed) and maximise the summed similarity; ties go to the smallest t_{m-1}, then
 * the smallest t_{m-2}, and so on.  The maximum is exact, so a plain f32 restatement gives the same bits whatever its scan order.
 * A constant added to a row does not move the path: it is also the Viterbi path under each row's log-softmax over time.
 *   rows [n_rows, 2] int32 (offset into sim, vlen) as for tan_window_stitch_final; order [n_rows] int32: packed row ids, a video's
 *   rows contiguous and in decode order; vtab [n_videos, 3] int32: first index into order, count, offset of the video's row in
 *   `run`; keep [n_rows] bytes indexed by packed row id (0 = the row is skipped while walking the video) or NULL = all.
 *   bp [n_acc] int32 (the back-pointers A, laid out like sim) and run [n_run] f32 (n_run >= sum of vlen: each video's M row,
 *   updated in place) are scratch and need no initialisation.
 *   ts [n_rows] int32 <- the second of every kept row, -1 for every other row a video lists (a row no video lists is not
 *   written); path [n_videos] f32 <- the path score, 0 for a video without a kept row.
 * Any vlen >= 1.  One workgroup per video, no atomics, no host synchronisation.  A video's rows share one vlen; a table entry that
 * points outside n_rows / n_acc / n_run, or a row of another vlen, takes no part (nothing is read or written out of bounds).
 * NULL pointers (other than keep) or non-positive counts: TAN_ERR_BAD_ARG, nothing launched.                                     */
int tan_monotonic_decode(const float* sim, const int* rows, const int* order, const int* vtab, int n_videos,
                         const unsigned char* keep, long n_rows, long n_acc, long n_run, int* bp, float* run, int* ts,
                         float* path, void* stream);
/* Aligned intervals: a segmental decode over the same stitched rows.  tan_monotonic_decode gives every kept sentence one second; this
 * gives it an inclusive interval [s, e], the intervals of one video decided together: ordered by decode order and disjoint.  Per video,
 * with its kept rows r_0 .. r_{m-1} in decode order, V = vlen, x_i[t] = sim[r_i][t] (as stitched, -6e4 cells included) and the gain
 * g_i[t] = x_i[t] - bias[r_i] (one f32 subtraction): segments [s_i, e_i] with s_i <= e_i and e_i < s_{i+1} (gaps allowed) that maximise
 * sum_i sum_{t in [s_i, e_i]} g_i[t].  As a recurrence (-inf is IEEE; every + is one f32 add, round to nearest, never contracted):
 *     G_{-1}[t] = 0 for t >= -1;   for i >= 0: G_i[-1] = -inf, E_i[-1] = -inf
 *     c = G_{i-1}[t-1];  p = E_i[t-1]
 *     E_i[t] = g_i[t] + max(p, c)              S_i[t] = t if c > p, else S_i[t-1]        (a tie extends the running segment)
 *     G_i[t] = max(G_i[t-1], E_i[t])           B_i[t] = the SMALLEST t' <= t with E_i[t'] == G_i[t]
 *     path = G_{m-1}[V-1];   e_{m-1} = B_{m-1}[V-1],  s_i = S_i[e_i],  e_{i-1} = B_{i-1}[s_i - 1]
 * E_i[t] (the best sum with sentence i's segment ending exactly at t) is finite exactly for t >= i; the problem is feasible iff
 * m <= V.  With exact sums the result is the optimum, and among optima the one with the smallest e_{m-1}, then the smallest s_{m-1},
 * then the smallest e_{m-2}, and so on; for m = 1 it is the maximum-sum run of g_0 (Kadane).  Every cell is one rounded add on top of
 * exact maxima and the dependency graph is fixed by the recurrence, so the bits of `path` and the segments do not depend on how the cells
 * are scheduled -- which is why it runs along t and is NOT restated as a prefix sum or a (max, +) scan: those re-associate the adds.
 *   sim, rows, order, vtab, keep, n_rows, n_acc, n_run: as for tan_monotonic_decode, with the same contract for a broken table entry
 *   (it takes no part; nothing is read or written out of bounds).  bias [n_rows] f32, by packed row id.
 *   bp [2 * n_acc] int32 (two planes laid out like sim: S_i[B_i[t]] and B_i[t]) and run [n_run] f32 (n_run >= sum of vlen: the G row
 *   one block of 256 sentences hands to the next) are scratch and need no initialisation.
 *   seg [n_rows, 2] int32 <- (s, e), inclusive, for every kept row; (-1, -1) for every other row a video lists (a row no video lists
 *   is not written).  path [n_videos] f32 <- the path score; 0 for a video without a kept row; -inf for a video with more kept rows
 *   than seconds, all of whose listed rows get (-1, -1).
 * Any vlen >= 1, any m.  One launch, one workgroup per video, no atomics, no host synchronisation.
 * NULL pointers (other than keep) or non-positive counts: TAN_ERR_BAD_ARG, nothing launched.                                       */
int tan_segment_decode(const float* sim, const int* rows, const int* order, const int* vtab, int n_videos,
                       const unsigned char* keep, const float* bias, long n_rows, long n_acc, long n_run, int* bp, float* run,
                       int* seg, float* path, void* stream);

/* ---- zero-shot retrieval (eval/eval_zeroshot_retrieval.py:13-27,157-256) and corpus search over a per-second index ----
 * tan_rank_topk: a matrix-free sweep over scores[q, n] = <Tq[q, :], Vn[n, :]>, Tq [Q, C], Vn [N, C], C == 512, both `dtype`
 * (TAN_BF16: bf16 operands, f32 accumulation; TAN_F32: exact-f32 MFMA), 16-byte aligned, rows prepared by the caller (normalised /
 * centred / standardised).  Nothing whose size grows with Q * N is stored.
 *   pair [Q] int32 or NULL: higher[q] / ties[q] (int32 [Q]) <- how many index rows score strictly above / exactly equal to the score
 *     of row pair[q] -- what compute_metrics (:13-27) reads off a sorted row.  The paired score is produced by the same instruction
 *     sequence as the sweep's own entry (q, pair[q]): ties[q] >= 1.  pair[q] in [0, N) is the CALLER's contract (the kernel clamps
 *     the address it reads, nothing more; the Python wrapper checks on request).  pair == NULL: higher / ties are not touched.
 *   k in [0, 32], k <= N: top_score / top_row [Q, k] <- the k best (score f32, row int32) per query by descending score, equal scores
 *     by ascending row; k == 0: counts only (then pair must be given; top_* may be NULL).
 *   splits: how many workgroups share the index per query tile of 128; 0 = chosen from Q and N, at most 256.  Counts, scores, rows
 *     and order are bit-identical from run to run and for every `splits`: per-split lists are merged by a total order in a second
 *     small launch, counts with integer atomics, no float atomics.
 *   ws: tan_rank_topk_ws_bytes(Q, N, k) bytes of scratch, 16-byte aligned (it does not depend on `splits`; -1 for invalid sizes).
 * Any Q >= 1, 1 <= N < 2^31; tails are masked in the kernel.  Another width, k > 32, k > N, bad sizes: TAN_ERR_BAD_ARG, nothing
 * launched.                                                                                                                       */
long tan_rank_topk_ws_bytes(long Q, long N, int k);
int tan_rank_topk(const void* Tq, const void* Vn, int dtype, long Q, long N, int C, const int* pair, int k, int splits,
                  int* higher, int* ties, float* top_score, int* top_row, void* ws, void* stream);
/* ---- the e4m3 index: 516 bytes per second of video instead of 1 KiB (model/tan_model.py:152, "can be used for retrieval
 * setting": the per-second index that tan_window_feat_* build, ranked by the sweep above) ----
 * Row format.  codes: OCP e4m3fn (gfx950's; NOT MI300's fnuz), one byte per element, [n_rows, 512].  scale: one f32 per row, a
 * power of two.  With amax = max|x| over the row and amax = m * 2^e, m in [0.5, 1) (frexp):
 *     s = e - 9 if m <= 0.875, else s = e - 8;  s is clamped to [-126, 127];  scale = 2^s;  amax == 0: scale = 1.
 * Hence |x / scale| <= 448 (e4m3fn's largest finite value): the conversion never saturates, and x * 2^-s is exact in f32.
 *     code = RNE_e4m3(x * 2^-s): round to nearest, ties to even, subnormals kept (the smallest is 2^-9) -- the function
 *     torch.Tensor.to(torch.float8_e4m3fn) computes on the host.
 * Inputs are finite.  A non-finite element is outside the contract: a NaN becomes a NaN code and makes every score of its row
 * NaN; an infinity sets the row's scale to 2^120, which flushes most of the row to zero, and its own code is unspecified.
 * Nothing is read or written out of bounds either way.
 * tan_quantize_rows_e4m3: x [n_rows, C] (TAN_F32 or TAN_BF16, 16-byte aligned), C == 512, 1 <= n_rows < 2^31 -> codes
 * [n_rows, 512] bytes (8-byte aligned), scale [n_rows].  One wave per row, no atomics: run-to-run identical.
 * tan_rank_topk_e4m3: tan_rank_topk over such rows -- Tq [Q, 512] / Vn [N, 512] codes (16-byte aligned), q_scale [Q] / v_scale
 * [N] their scales.  score(q, n) = (acc * v_scale[n]) * q_scale[q], with acc the f32 accumulation of the code products by
 * v_mfma_f32_32x32x16_fp8_fp8 and the two multiplies in f32, in that order, in the pair launch and in the sweep alike: the
 * sweep's own entry (q, pair[q]) has the pair score's bits, ties[q] >= 1.  pair / k / splits / higher / ties / top_score / top_row
 * / ws (tan_rank_topk_ws_bytes(Q, N, k)), determinism and argument rules: exactly as tan_rank_topk.                               */
int tan_quantize_rows_e4m3(const void* x, int dtype, long n_rows, int C, void* codes, float* scale, void* stream);
int tan_rank_topk_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Q, long N, int C,
                       const int* pair, int k, int splits, int* higher, int* ties, float* top_score, int* top_row, void* ws,
                       void* stream);
/* ---- the coarse image: 272 bytes per second of video in MXFP4, the block-scaled 4-bit format gfx950 multiplies natively
 * (v_mfma_scale_f32_32x32x64_f8f6f4) -- what `search(..., coarse=)` sweeps on the card before the exact sweep rescores its candidates ----
 * Row format.  A row of 512 elements is 16 blocks of 32 consecutive elements.  codes: uint8 [n_rows, 256], two e2m1 codes per byte;
 * scales: uint8 [n_rows, 16], one e8m0 byte per block; both contiguous.
 *   Block scale.  With amax = max|x| over the block and amax = m * 2^e, m in [0.5, 1) (frexp):
 *       s = e - 3 if m <= 0.75, else s = e - 2;  s is clamped to [-127, 127];  the byte is s + 127;  amax == 0: the byte is 127.
 *     Hence amax * 2^-s lies in (3, 6] (6 is e2m1's largest value): a block never saturates, as an e4m3 row never does.  The NaN
 *     byte 255 is never written.
 *   Code.  code = RNE_e2m1(x * 2^-s): the magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6 are the codes 0 .. 7 in bits 0 to 2; round to
 *     nearest, ties to the even code: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4.  Bit 3 is the sign
 *     bit of x, whatever the magnitude rounds to: a negative element that rounds to zero, and -0.0 itself, have the code 8 (the
 *     instruction reads it as zero).
 *   Nibble order.  Element 2 j of a row is the LOW nibble (bits 0 to 3) of byte j, element 2 j + 1 the high one: the order in
 *     which the scaled MFMA consumes a 4-bit operand, so the 16 bytes of a block go into a lane's operand registers unpermuted
 *     (pinned with exact data by tests/test_coarse_gpu.py).
 *   Inputs are finite; x * 2^-s is exact apart from f32 underflow, which rounds to the code 0 either way.
 * tan_quantize_rows_mxfp4: x [n_rows, C] (TAN_F32 or TAN_BF16, 16-byte aligned), C == 512, 1 <= n_rows < 2^31 -> codes (4-byte
 *   aligned) and scales.  One wave per row, a block is four lanes, no atomics: run-to-run identical.
 * tan_rank_topk_mxfp4: the k best rows per query of such an image.  The QUERY keeps the e4m3 row format above (Tq [Q, 512] codes,
 *   16-byte aligned, q_scale [Q]); codes [N, 256] and scales [N, 16] are 16-byte aligned.
 *       score_c(q, n) = (sum over blocks b of 2^s[n][b] * sum over i in b of qcode[q][i] * vcode[n][i]) * q_scale[q]
 *   accumulated in f32 by v_mfma_scale_f32_32x32x64_f8f6f4 in ascending K order (the image is the fp4 operand with its block scales
 *   in the instruction's scale operand, the query the fp8 operand with scale 2^0), then ONE f32 multiply by q_scale[q].
 *   top_score / top_row [Q, k] <- per query the k best (score_c, row) by descending score, equal scores by ascending row.
 *   Cutoff.  below_score / below_row [Q] (f32 / int32), both NULL or both given: a row is admitted only when it comes STRICTLY AFTER
 *     (below_score[q], below_row[q]) in that order -- score_c < below_score[q], or equal and row > below_row[q].  A cutoff row of -1
 *     admits every row at an equal score, 0x7fffffff none.  So a list continues: two calls with k = 16, the second cut off below
 *     the first's last entry, give exactly the one call with k = 32.  With fewer than k admitted rows the tail holds empty slots
 *     (-inf, row 0x7fffffff), which tan_topk_fold sorts last.
 *   1 <= k <= 32, k <= N; splits, determinism (bit-identical for every `splits`) and sizes as tan_rank_topk.
 *   ws: tan_rank_topk_mxfp4_ws_bytes(Q, N, k) bytes of scratch, 16-byte aligned (-1 for invalid sizes).
 *   NULL pointers, another width, bad sizes or alignment: TAN_ERR_BAD_ARG, nothing launched.                                       */
int tan_quantize_rows_mxfp4(const void* x, int dtype, long n_rows, int C, void* codes, void* scales, void* stream);
long tan_rank_topk_mxfp4_ws_bytes(long Q, long N, int k);
int tan_rank_topk_mxfp4(const void* Tq, const float* q_scale, const void* codes, const void* scales, long Q, long N, int C, int k,
                        int splits, const float* below_score, const int* below_row, float* top_score, int* top_row, void* ws,
                        void* stream);
/* ---- moment search: the k best DISTINCT videos per query, each with its best second and the extent of the moment around it ----
 * tan_rank_topk_video: tan_rank_topk's sweep (Tq [Q, C], Vn [N, C], C == 512, `dtype` TAN_F32 or TAN_BF16, 16-byte aligned) over
 * an index whose rows are grouped into videos: v_off [n_videos + 1] int32 on the device, v_off[0] == 0, v_off[n_videos] == N,
 * strictly increasing (video v owns the rows [v_off[v], v_off[v + 1]); every video has at least one row); 1 <= n_videos <= N.
 *   top_score / top_row / top_video [Q, k], 1 <= k <= 32, k <= n_videos: the k videos with the largest
 *     max over n in [v_off[v], v_off[v + 1]) of score(q, n), by descending maximum, equal maxima by ascending top_row (videos are
 *     contiguous row ranges, so that is ascending video number too).  top_score (f32) is that maximum, top_row (int32) the
 *     SMALLEST row of v that attains it -- a global index row; the second is top_row - v_off[v] -- and top_video (int32) is v.
 *   score(q, n) comes from the same instruction sequence as tan_rank_topk's sweep (the same MFMA chains in the same order): the
 *     returned scores have that sweep's bits.  Nothing whose size grows with Q * N or Q * n_videos is stored.
 *   splits: as tan_rank_topk.  Scores, rows, videos and order are bit-identical from run to run and for every `splits`; a video
 *     may straddle 64-row tiles and split boundaries.  No float atomics.
 *   ws: tan_rank_topk_video_ws_bytes(Q, N, n_videos, k) bytes of scratch, 16-byte aligned: the videos of every 64-row tile's first and
 *     last row (N / 8 bytes) and the splits' lists (at most 256 * Q * k * 12 bytes); it does not depend on `splits`; -1 for invalid
 *     sizes.
 * A v_off that breaks its contract is the CALLER's error: every video lookup is clamped to [0, n_videos), nothing is read or
 * written out of bounds, and the lists are unspecified (a slot may then hold score -inf, row 0x7fffffff, video -1).  The Python
 * wrapper checks v_off on request.
 * Any Q >= 1, 1 <= N < 2^31; tails are masked in the kernel.  Another width, k outside [1, min(32, n_videos)], an unknown dtype, a
 * NULL pointer, negative splits, n_videos outside [1, N]: TAN_ERR_BAD_ARG, nothing launched.
 * tan_rank_topk_video_e4m3: the same over the e4m3 rows of tan_rank_topk_e4m3, score(q, n) = (acc * v_scale[n]) * q_scale[q].
 * tan_moment_extent / _e4m3: for every hit (q, i) of such lists (top_score / top_row / top_video [Q, k], the same Tq, Vn, v_off,
 * n_videos, k) and width >= 0 (f32): start / end [Q, k] int32 <- the moment around the peak as GLOBAL index rows, inclusive.  With
 * p = top_row[q, i], v = top_video[q, i] and thr = top_score[q, i] - width (one f32 subtraction):
 *     start = the smallest row >= v_off[v] such that every row n in [start, p) has s(q, n) >= thr,
 *     end   = the largest row < v_off[v + 1] such that every row n in (p, end] has s(q, n) >= thr;
 * row p itself is inside and is not tested again.  s(q, n) is the f32 dot product of the stored operands (bf16 / f32 values, or
 * e4m3 codes with (acc * v_scale[n]) * q_scale[q]) in this kernel's own summation order; it need not have the sweep's bits.  One
 * wave per hit walks outward from p and stops at the first failing row: the cost follows the moment's length, any vlen >= 1, no
 * scratch, no atomics, run-to-run identical.  A top_row / top_video outside the index is clamped for memory safety and gives
 * unspecified extents.  Argument rules as tan_rank_topk_video (no splits, no ws), and width < 0 or NaN: TAN_ERR_BAD_ARG.         */
long tan_rank_topk_video_ws_bytes(long Q, long N, long n_videos, int k);
int tan_rank_topk_video(const void* Tq, const void* Vn, int dtype, long Q, long N, int C, const int* v_off, long n_videos, int k,
                        int splits, float* top_score, int* top_row, int* top_video, void* ws, void* stream);
int tan_rank_topk_video_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Q, long N, int C,
                             const int* v_off, long n_videos, int k, int splits, float* top_score, int* top_row, int* top_video,
                             void* ws, void* stream);
int tan_moment_extent(const void* Tq, const void* Vn, int dtype, long Q, long N, int C, const int* v_off, long n_videos, int k,
                      const float* top_score, const int* top_row, const int* top_video, float width, int* start, int* end,
                      void* stream);
int tan_moment_extent_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Q, long N, int C,
                           const int* v_off, long n_videos, int k, const float* top_score, const int* top_row,
                           const int* top_video, float width, int* start, int* end, void* stream);
/* ---- ordered-sequence search: the k videos that show a list of steps in order, by their best order-preserving path ----
 * A SEQUENCE is 1 to 32 consecutive rows of Tq [Qt, C] (its steps, in order): s_off [n_seq + 1] int32 on the device, s_off[0] == 0,
 * s_off[n_seq] == Qt, strictly increasing, every difference in [1, 32].  A VIDEO v is the index rows [v_off[v], v_off[v + 1]) -- the
 * v_off contract of tan_rank_topk_video.  For sequence p with steps q_0 .. q_{m-1} and video v with V rows, let
 * x_i[t] = score(q_i, v_off[v] + t).  Then
 *     D_0[t] = x_0[t];   D_i[t] = x_i[t] + M_{i-1}[t]   -- one f32 add, round to nearest, never contracted
 *     M_i[t] = max_{t' <= t} D_i[t'];   path(p, v) = M_{m-1}[V - 1]
 * -- tan_monotonic_decode's recurrence, word for word: non-decreasing seconds, equal seconds allowed, any V >= 1, also V < m.  The
 * maximum is exact and each cell is one rounded add, so given the bits of x the bits of path do not depend on scan order, tiling or
 * splits.  score(q, n) is the row sweep's: the MFMA chain of tan_rank_topk in the same K order (e4m3: (acc * v_scale[n]) *
 * q_scale[q]); an MFMA element does not depend on where its row sits in a tile, so a video is tiled from its own first row.
 * tan_sequence_topk (Tq, Vn, dtype, C == 512, alignment as tan_rank_topk):
 *   top_score / top_video [n_seq, k], 1 <= k <= min(32, n_videos): per sequence the k videos with the largest path(p, v), by
 *     descending path, equal paths by ascending video.  top_score (f32) is the path, top_video (int32) is v.
 *   splits: how many workgroups share the index per four sequences; 0 = chosen from n_seq and N, at most 256.  A split takes WHOLE
 *     videos (those whose first row falls into its row range).  Results are bit-identical from run to run and for every `splits`;
 *     no float atomics.  Nothing of size Qt x N, n_seq x N or n_seq x n_videos is stored.
 *   ws: tan_sequence_topk_ws_bytes(n_seq, N, k) bytes of scratch, 16-byte aligned: the splits' lists (at most 256 * n_seq * k * 8
 *     bytes; the splits' video ranges are searched in v_off by the kernel); it does not depend on `splits`; -1 for invalid sizes.
 * Another width, k outside [1, min(32, n_videos)], an unknown dtype, a NULL pointer, misalignment, negative splits, n_seq < 1, Qt
 * outside [n_seq, 32 * n_seq], n_videos outside [1, N], N outside [1, 2^31): TAN_ERR_BAD_ARG, nothing launched.
 * An s_off or v_off that breaks its contract is the CALLER's error: every lookup is clamped, nothing is read or written out of
 * bounds, and the lists are unspecified (a slot may then hold score -inf, video 0x7fffffff).  The Python wrapper checks on request.
 * tan_sequence_scores: for P hits, hits [P, 2] int32 = (sequence, video) on the device, x + x_off[h] <- x_i[t], i < m, t < V,
 * row-major [m, V] f32 (x_off [P]: `long` element offsets on the device, x holds n_x elements) -- the scores with the bits
 * tan_sequence_topk used (the same tile routine, the same K order).  A hit whose sequence or video lies outside the tables, or whose
 * block would leave [0, n_x), is skipped.  One workgroup per hit, no atomics.  tan_monotonic_decode over such a block (one "video" of
 * its tables per hit, the hit's m rows in step order) returns the path's seconds, and its `path` equals top_score bit for bit.
 * The _e4m3 variants take the codes and scales of tan_rank_topk_e4m3.                                                              */
long tan_sequence_topk_ws_bytes(long n_seq, long N, int k);
int tan_sequence_topk(const void* Tq, const void* Vn, int dtype, long Qt, long N, int C, const int* s_off, long n_seq,
                      const int* v_off, long n_videos, int k, int splits, float* top_score, int* top_video, void* ws, void* stream);
int tan_sequence_topk_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Qt, long N, int C,
                           const int* s_off, long n_seq, const int* v_off, long n_videos, int k, int splits, float* top_score,
                           int* top_video, void* ws, void* stream);
int tan_sequence_scores(const void* Tq, const void* Vn, int dtype, long Qt, long N, int C, const int* s_off, long n_seq,
                        const int* v_off, long n_videos, const int* hits, const long* x_off, long P, float* x, long n_x,
                        void* stream);
int tan_sequence_scores_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Qt, long N, int C,
                             const int* s_off, long n_seq, const int* v_off, long n_videos, const int* hits, const long* x_off,
                             long P, float* x, long n_x, void* stream);
/* ---- clip search: the k videos in which a piece of video appears, second for second, and where ----
 * A CLIP is 1 to 32 consecutive rows of Tq [Qt, C] (its seconds, in order): c_off [n_clip + 1] int32 on the device, c_off[0] == 0,
 * c_off[n_clip] == Qt, strictly increasing, every difference in [1, 32] -- the contract of s_off.  A VIDEO v is the index rows
 * [v_off[v], v_off[v + 1]) -- the v_off contract of tan_rank_topk_video.  For clip p with rows q_0 .. q_{m-1} and video v with V rows,
 * let x_i[t] = score(q_i, v_off[v] + t), the row sweep's score: the MFMA chain of tan_rank_topk in the same K order (e4m3:
 * (acc * v_scale[n]) * q_scale[q]).  Then
 *     S(t)        = (((x_0[t] + x_1[t + 1]) + x_2[t + 2]) + ... ) + x_{m-1}[t + m - 1]        for 0 <= t <= V - m
 *     match(p, v) = max_t S(t);   start(p, v) = the smallest t attaining it
 * -- the clip laid over the video second for second, not tan_sequence_topk's non-decreasing seconds.  Every + is one f32 add, round
 * to nearest, never contracted, in ascending i; the maximum is exact and the add order is fixed, so given the bits of x the bits of
 * S do not depend on tiling, splits or shards.  A video with V < m has no start and is not a candidate.  Inputs are finite.
 * tan_sequence_scores with c_off as its s_off returns x with the bits this sweep uses (videos are tiled from their own first row by
 * the same routine).
 * tan_clip_topk (Tq, Vn, dtype, C == 512, alignment as tan_rank_topk):
 *   top_score (f32) / top_row / top_video (int32) [n_clip, k], 1 <= k <= min(32, n_videos): per clip the k videos with the largest
 *     match(p, v), by descending match, equal matches by ascending row.  top_score is the SUM S (not the mean), top_row =
 *     v_off[v] + start(p, v) -- a global index row -- and top_video is v.  When fewer than k videos hold m rows, the remaining
 *     slots are (-inf, 0x7fffffff, -1): the empty slots of the filtered sweeps, which tan_topk_fold sorts last.
 *   splits: as tan_sequence_topk: a split takes WHOLE videos (those whose first row falls into its row range), 0 = chosen from
 *     n_clip and N, at most 256.  Results are bit-identical from run to run and for every `splits`; no float atomics.  Nothing of
 *     size Qt x N, n_clip x N or n_clip x n_videos is stored.
 *   ws: tan_clip_topk_ws_bytes(n_clip, N, k) bytes of scratch, 16-byte aligned: the splits' lists of (score, row, video) only (at
 *     most 256 * n_clip * k * 12 bytes); it does not depend on `splits`; -1 for invalid sizes.
 * Another width, k outside [1, min(32, n_videos)], an unknown dtype, a NULL pointer, misalignment, negative splits, n_clip < 1, Qt
 * outside [n_clip, 32 * n_clip], n_videos outside [1, N], N outside [1, 2^31): TAN_ERR_BAD_ARG, nothing launched.
 * A c_off or v_off that breaks its contract is the CALLER's error: every lookup is clamped (a clip of more than 32 rows is cut to
 * 32), nothing is read or written out of bounds, and the lists are unspecified.  The Python wrapper checks on request.
 * tan_clip_topk_e4m3 takes the codes and scales of tan_rank_topk_e4m3.                                                            */
long tan_clip_topk_ws_bytes(long n_clip, long N, int k);
int tan_clip_topk(const void* Tq, const void* Vn, int dtype, long Qt, long N, int C, const int* c_off, long n_clip, const int* v_off,
                  long n_videos, int k, int splits, float* top_score, int* top_row, int* top_video, void* ws, void* stream);
int tan_clip_topk_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Qt, long N, int C,
                       const int* c_off, long n_clip, const int* v_off, long n_videos, int k, int splits, float* top_score,
                       int* top_row, int* top_video, void* ws, void* stream);
/* ---- compound search: the k videos that satisfy AND / OR / NOT of query rows, in any order ----
 * A COMPOUND QUERY is 1 to 32 consecutive rows of Tq [Qt, C], its TERMS: t_off [n_query + 1] int32 on the device, t_off[0] == 0,
 * t_off[n_query] == Qt, strictly increasing, every difference in [1, 32] -- the contract of s_off.  role [Qt] int32 on the device gives
 * every term its part: j in [0, 31] = the term belongs to CLAUSE j, -1 = the term is BANNED; every query has at least one clause
 * term.  One float `veto` holds for the whole call.  A VIDEO v is the index rows [v_off[v], v_off[v + 1]) -- the v_off contract of
 * tan_rank_topk_video.  For a video v with at least one row and a term t, let x[t, n] = score(q_t, n), the row sweep's score: the
 * MFMA chain of tan_rank_topk in the same K order (e4m3: (acc * v_scale[n]) * q_scale[t]).  Inputs are finite.  Then
 *     peak    p_t = x[t, r_t], r_t = the first row n of v, ascending, that no other row of v beats under float > -- the value AT that
 *                   row, not a max() that might pick the other zero of +-0
 *     clause  g_j = p_t of the first term t of clause j, in term order, that no other term of the clause beats under >         (OR)
 *     score       = the occupied clauses folded in ascending j, starting from the first one; the running value is replaced only
 *                   under strict <                                                                (AND: the weakest link)
 *     veto        : a video with p_t >= veto for any banned term t is not a candidate; without banned terms pass +inf    (NOT)
 * A video without rows is never a candidate.  Maxima and minima are exact, so given the bits of x nothing depends on tiling,
 * splits or shards.
 * tan_compound_topk (Tq, Vn, dtype, C == 512, alignment as tan_rank_topk):
 *   top_score (f32) / top_video (int32) [n_query, k], 1 <= k <= min(32, n_videos): per query the k candidates with the largest
 *     score, by descending score, equal scores by ascending video.  With fewer than k candidates the tail is (-inf, 0x7fffffff):
 *     the empty slots of tan_clip_topk, which tan_topk_fold sorts last.
 *   splits: as tan_sequence_topk: a split takes WHOLE videos (those whose first row falls into its row range), 0 = chosen from
 *     n_query and N, at most 256.  Results are bit-identical from run to run and for every `splits`; no float atomics.  Nothing of
 *     size Qt x N, n_query x N or n_query x n_videos is stored.
 *   ws: tan_compound_topk_ws_bytes(n_query, N, k) bytes of scratch, 16-byte aligned: the splits' lists (at most 256 * n_query * k * 8
 *     bytes); it does not depend on `splits`; -1 for invalid sizes.
 * tan_compound_peaks: for n_hits hits, hits [n_hits, 2] int32 = (query, video) on the device, peak_score f32 / peak_row int32
 * [n_hits, 32] <- (p_t, r_t) of the query's term t in column t, r_t a GLOBAL index row, with the bits tan_compound_topk used (the
 * same routine); columns >= the query's number of terms, and every column of a hit whose query or video lies outside the tables or
 * whose video has no row, hold (-inf, 0x7fffffff): every element is written.  One workgroup per hit, no atomics, no scratch.
 * Another width, k outside [1, min(32, n_videos)], a NaN veto, an unknown dtype, a NULL pointer, misalignment, negative splits,
 * n_query < 1, Qt outside [n_query, 32 * n_query], n_videos outside [1, N], N outside [1, 2^31), n_hits outside [1, 2^26):
 * TAN_ERR_BAD_ARG, nothing launched.  A t_off, role or v_off that breaks its contract is the CALLER's error: every lookup is clamped
 * (a query of more than 32 terms is cut to 32, a role below -1 counts as banned, a query without a clause term has no candidate),
 * nothing is read or written out of bounds, and the lists are unspecified.  The Python wrapper checks on request.
 * The _e4m3 variants take the codes and scales of tan_rank_topk_e4m3.                                                              */
long tan_compound_topk_ws_bytes(long n_query, long N, int k);
int tan_compound_topk(const void* Tq, const void* Vn, int dtype, long Qt, long N, int C, const int* t_off, const int* role,
                      long n_query, const int* v_off, long n_videos, float veto, int k, int splits, float* top_score, int* top_video,
                      void* ws, void* stream);
int tan_compound_topk_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Qt, long N, int C,
                           const int* t_off, const int* role, long n_query, const int* v_off, long n_videos, float veto, int k,
                           int splits, float* top_score, int* top_video, void* ws, void* stream);
int tan_compound_peaks(const void* Tq, const void* Vn, int dtype, long Qt, long N, int C, const int* t_off, long n_query,
                       const int* v_off, long n_videos, const int* hits, long n_hits, float* peak_score, int* peak_row, void* stream);
int tan_compound_peaks_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Qt, long N, int C,
                            const int* t_off, long n_query, const int* v_off, long n_videos, const int* hits, long n_hits,
                            float* peak_score, int* peak_row, void* stream);
/* ---- cover search: the k videos that share the most seconds with a set of query rows, in any order and at any pace ----
 * A SET is 1 to 4096 (tan_cover_max_rows()) consecutive rows of Tq [Qt, C]: q_off [n_set + 1] int32 on the device, q_off[0] == 0,
 * q_off[n_set] == Qt, strictly increasing, every difference in [1, 4096].  A VIDEO v is the index rows [v_off[v], v_off[v + 1]) -- the
 * v_off contract of tan_rank_topk_video.  For set p with rows q_0 .. q_{m-1} and video v with V rows, let
 * x_i[t] = score(q_i, v_off[v] + t), the row sweep's score with the bits tan_sequence_scores returns (e4m3:
 * (acc * v_scale[n]) * q_scale[q]).  Inputs are finite.  The measure is the Chamfer similarity of the two sets of rows:
 *     a_i  = max_t x_i[t]          b_t = max_i x_i[t]                       (exact)
 *     fix(x) = __float2ll_rn(x * 2^30)                                      (tan_cluster_accumulate's image; the multiply is exact)
 *     F = sum_i fix(a_i)           B = sum_t fix(b_t)                       (64-bit integers: order-free)
 *     fwd(p, v) = ((float) F * 2^-30f) / (float) m                          (int64 -> f32 round to nearest even, exact scaling, ONE f32 division)
 *     bwd(p, v) = ((float) B * 2^-30f) / (float) V
 *     score = fwd                    rank == TAN_COVER_QUERY  ("how much of my video is in v")
 *           = bwd                    rank == TAN_COVER_VIDEO  ("how much of v is in my video")
 *           = (fwd + bwd) * 0.5f     rank == TAN_COVER_BOTH   (one f32 add, one exact multiply)
 * |x| <= 2 and m, V < 2^31, so no sum overflows.  Given the bits of x, nothing depends on tiling, slabs, launch shape or shards.
 * tan_cover_topk (Tq, Vn, dtype, C == 512, alignment as tan_rank_topk):
 *   fwd / bwd [n_set, n_videos] f32, caller-owned, always fully written: the all-pairs result and the only storage that grows with
 *     n_set * n_videos.  Nothing of size Qt x N, n_set x N or Qt x n_videos is stored; no scratch, no atomics in global memory,
 *     run-to-run identical bits.
 *   top_score (f32) / top_row / top_video (int32) [n_set, k], 1 <= k <= min(32, n_videos): per set the k videos by descending score,
 *     equal scores by ascending top_row = v_off[v] -- the sweeps' order, so tan_topk_fold folds the lists as they are.
 * 1 <= n_set <= 65535, Qt in [n_set, 4096 n_set], 1 <= N < 2^31, n_videos in [1, N].  Another width, k outside [1, min(32, n_videos)],
 * an unknown dtype or rank, a NULL pointer, misalignment, sizes outside these ranges: TAN_ERR_BAD_ARG, nothing launched.
 * A q_off or v_off that breaks its contract is the CALLER's error: every lookup is clamped (a set of more than 4096 rows is cut to
 * 4096; an empty video gets fwd = bwd = 0), nothing is read or written out of bounds, and the results are unspecified.  The Python
 * wrapper checks on request.  tan_cover_topk_e4m3 takes the codes and scales of tan_rank_topk_e4m3.                              */
#define TAN_COVER_QUERY 0
#define TAN_COVER_VIDEO 1
#define TAN_COVER_BOTH 2
int tan_cover_max_rows(void);                      /* 4096 */
int tan_cover_topk(const void* Tq, const void* Vn, int dtype, long Qt, long N, int C, const int* q_off, long n_set, const int* v_off,
                   long n_videos, int rank, int k, float* fwd, float* bwd, float* top_score, int* top_row, int* top_video,
                   void* stream);
int tan_cover_topk_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Qt, long N, int C,
                        const int* q_off, long n_set, const int* v_off, long n_videos, int rank, int k, float* fwd, float* bwd,
                        float* top_score, int* top_row, int* top_video, void* stream);
/* Clip pooling of test_retrieval_yc2 (:197-214).  stage: one stage of the video stack's output, window w's frame f at
 * stage + w * win_stride + f * 512 elements of `dtype` (win_stride >= T * 512, a multiple of 8); table [W, 3] int32 = (clip,
 * first_frame, n_frames) per window.  normalize != 0: every selected frame is L2-normalised (sim = 'cos').  sum [n_clips, 512] /
 * cnt [n_clips] f32 += the frames / their number; the windows of a clip may come in several calls.  Within a call the first window
 * naming a clip adds all of them in window order (no float atomics).  _final: out [n_clips, 512] f32 = sum / cnt -- the
 * reference's mean over windows of the mean over frames, a clip's windows holding equally many frames -- L2-normalised again when
 * normalize != 0.                                                                                                                */
int tan_segment_pool_acc(const void* stage, int dtype, long win_stride, int T, const int* table, int W, int normalize, float* sum,
                         float* cnt, int n_clips, void* stream);
int tan_segment_pool_final(const float* sum, const float* cnt, int n_clips, int normalize, float* out, void* stream);
/* The per-second index: the feature counterpart of tan_window_stitch_acc / _final.  feat: the last video stage of a pass's windows
 * (addressing as above); table: the pass's TAN_WIN_FIELDS rows, of which vrow (index row of the window's first frame) and t are
 * read.  acc [n_rows, 512] / cnt [n_rows] f32 += every covering window's L2-normalised frame row / 1, the first covering window of
 * the pass adding all of them in window order.  _final: out [n_rows, 512] (TAN_BF16 or TAN_F32) = acc / max(cnt, 1).  The text
 * side of the dual similarity is one unit vector t_hat in every window, so <out[g], t_hat> / 0.07 is the stitched dual similarity
 * acc_d / cnt of eval_zeroshot_align.py:198,201.                                                                                 */
int tan_window_feat_acc(const void* feat, int dtype, long win_stride, const int* table, int W, int T, float* acc, float* cnt,
                        long n_rows, void* stream);
int tan_window_feat_final(const float* acc, const float* cnt, long n_rows, void* out, int out_dtype, void* stream);

/* ---- two-stage search: the dual sweep's candidates rescored by the joint stack (`search.search_rerank`) ----
 * tan_rerank_tail: one (score, second, confidence, alignability) per window from a pass of joint-stack outputs.
 *   stage_last: the last joint stage after ln_joint_post_enc, [W, L, 512] of `dtype` (TAN_F32 or TAN_BF16), 16-byte aligned; window
 *     w's frame f is row w * L + f, f < T, and its query is the text row w * L + T (the first text slot; L > T, 1 <= T <= 1024).
 *   stage_head: joint stage index 2 in the same layout (what eval_zeroshot_align.py:186 reads; it may be stage_last itself), or NULL.
 *   table: the pass's TAN_WIN_FIELDS rows, of which t and s0 are read; t is clamped to [0, T].
 *   Per window, in f32, a lane of the wave owning channels 8 lane .. 8 lane + 7:
 *     dot(a, b) = wave_sum(the lane's 8 products added in channel order)   -- wave_sum: tan_common.h's fixed 64-lane tree
 *     cos[f] = dot(v_f, q) / (sqrtf(dot(v_f, v_f)) * sqrtf(dot(q, q)))     for f < t; no epsilon, as tan_model.py:116-117,136-137
 *     out[4 w + 0] = max_f cos[f]                        (NaN cosines are passed over)
 *     out[4 w + 1] = s0 + the FIRST f attaining it, an int32 stored as its bit pattern in the f32 slot
 *     out[4 w + 2] = 1 / sum_f expf(cos[f] / 0.07f - max / 0.07f)          -- the maximum of the softmax over the t valid frames of
 *                    cos / 0.07 (align_corpus's `confidence`); a lane adds its frames f = lane, lane + 64, .. in order, then wave_sum
 *     out[4 w + 3] = dot(head_w, text row of stage_head) + head_b[0]       (tan_model.py:148), 0 when stage_head is NULL
 *   t >= 1 is the caller's contract; t <= 0 gives (-inf, s0, 0, .).  sim [W, T] f32 or NULL: cos[f], -inf for f >= t.
 *   Error against the exact cosine of the same stored rows: each of the three dots is a 512-term f32 accumulation, error at most
 *   512 * 2^-23 * sum_i |a_i b_i| (bound (a) of DESIGN 3.12); the two square roots halve the norms' relative error and add 2^-24
 *   each, the product and the division 2^-24 each.  With A = sum_i |v_i q_i| / (|v| |q|) <= 1:
 *       |cos - exact| <= 2^-23 * (512 A + 516 |cos|)  <=  1028 * 2^-23 = 1.23e-4.
 *   One workgroup per window; every stage row is read once, by one wave, with 16-byte loads; the four outputs leave in one 16-byte
 *   store.  No atomics, no scratch: a window's bits depend on its rows alone, not on W or on the windows around it.
 *   NULL stage_last / table / out, stage_head without head_w / head_b, misalignment, sizes outside the above: TAN_ERR_BAD_ARG.
 * tan_rerank_select: score(q, i) = score[(q * P + i) * stride] (f32; stride = 4 reads tan_rerank_tail's out), 1 <= P <= 32,
 *   1 <= k <= P, Q >= 1: out_idx [Q, k] int32 <- the k candidates i of query q with the largest score, by descending score, equal
 *   scores by ascending i (candidates arrive in dual rank order, so ties keep it); a NaN score counts as -inf.  One wave per query
 *   through the rank sweeps' sort64.  Bad sizes or NULL pointers: TAN_ERR_BAD_ARG.                                                  */
int tan_rerank_tail(const void* stage_last, const void* stage_head, int dtype, int L, int T, const int* table, int W,
                    const float* head_w, const float* head_b, float* out, float* sim, void* stream);
int tan_rerank_select(const float* score, long Q, int P, long stride, int k, int* out_idx, void* stream);

/* ---- sharded search: the device fold of per-shard top-k lists (`search.ShardedIndex`) ----
 * An index cut into shards (whole videos each) is swept shard by shard; the sweeps above leave per-shard lists whose rows / videos
 * count from the shard's own start.  Three of their contracts make the sharded answer exact: a score does not depend on where its
 * row sits in a tile, a split or an index (tan_rank_topk); a path depends only on the bits of its video's scores
 * (tan_sequence_topk); tan_moment_extent reads only its own video's rows.
 * tan_topk_fold: run_score (f32) / run_shard / run_row (int32) [Q, k] and run_aux [n_aux, Q, k] int32 (NULL when n_aux == 0) hold a
 * running list per query; in_score / in_row [Q, k_in] and in_aux0 .. in_aux2 [Q, k_in] int32 (the first n_aux non-NULL, the rest
 * ignored) are the list of shard number `shard`.
 *   Result: run_*[q, :] <- the k best of (old run list of q) U (incoming list of q, each entry with shard `shard`) under the TOTAL
 *     order score descending, then shard ascending, then row ascending -- with row_base[shard] the rows before the shard, the
 *     sweeps' order on the global row row_base[shard] + row (or on the global video number, where `row` carries a video).
 *   Payload: the aux columns travel with their entry unchanged (moment search: the video and the extent's start and end).
 *   reset != 0: the old content of run_* is not read; the run list counts as empty.
 *   Empty slots: an empty run slot is (-inf, shard 0x7fffffff, row 0x7fffffff, aux -1); an incoming slot whose row is 0x7fffffff
 *     (what the sweeps leave under a broken v_off) counts as empty whatever its score; empty slots sort last.  With fewer than k
 *     entries in all, the tail of the run list is empty slots.
 *   Order independence: the order is total on (shard, row) and taking the k best of a union is associative and commutative, so
 *     the run list after folding every shard ONCE does not depend on the order of the folds.  Folding a shard twice is the caller's
 *     error (its entries then appear twice).
 *   1 <= Q < 2^31, 1 <= k <= 32, 1 <= k_in <= k, 0 <= n_aux <= 3, 0 <= shard < 2^31 - 1.  The incoming arrays must not overlap
 *     the run arrays; the fold is in place on the run arrays.
 *   One wave per query, four queries per 256-thread workgroup; lanes 0..31 hold the run list, lanes 32..63 the incoming one, one
 *     64-lane sorting network under the three-part key, payload by one cross-lane move per column.  No atomics, no scratch, no LDS:
 *     run-to-run identical.
 *   A NULL run_score / run_shard / run_row / in_score / in_row, run_aux NULL with n_aux > 0, one of the first n_aux in_aux pointers
 *     NULL, sizes outside the ranges: TAN_ERR_BAD_ARG, nothing launched.                                                          */
int tan_topk_fold(float* run_score, int* run_shard, int* run_row, int* run_aux, long Q, int k, int n_aux, int reset,
                  const float* in_score, const int* in_row, const int* in_aux0, const int* in_aux1, const int* in_aux2, int k_in,
                  int shard, void* stream);

/* ---- filtered search: a sweep restricted to row spans (`search.RowFilter`: a playlist, an exclusion list, time windows) ----
 * A FILTER over an index of N rows is a list of row spans [lo, hi): spans [n_spans, 2] int32 on the device, ascending, disjoint,
 * non-empty, inside [0, N).  Rows inside a span are ADMITTED.  A sweep reads a filter through its IMAGE:
 * tan_row_filter_build: spans -> the image, in caller-owned device memory `filt` of tan_row_filter_bytes(N) bytes (16-byte
 *   aligned; -1 for N outside [1, 2^31)).  With T = ceil(N / 64) 64-row tiles, T2 = T rounded up to 2, in int32 words:
 *     [0]                     n_listed: how many tiles hold an admitted row
 *     [1]                     T;  [2], [3]: 0
 *     [4, 4 + T2)             the listed tiles' numbers, ascending (the first n_listed entries; the rest is not written)
 *     [4 + T2, 4 + T2 + 2 T)  one 64-bit row mask per LISTED tile, in list order: bit r set <=> row 64 * tile + r is admitted
 *                             (never a row >= N)
 *     the rest                scratch of the build (every tile's mask, then one count per 256 tiles); no sweep reads it
 *   Three launches: a thread per tile finds the spans that meet its tile by binary search and counts per block, one block scans
 *   the counts, a thread per tile writes its list entry.  No atomics: the image is bit-identical from run to run.  The same image
 *   serves every Q, k, splits and row format of an index of N rows.
 *   Spans that break their contract are the CALLER's error: every span is cut to its tile and to [0, N), at most 64 spans are
 *   looked at per tile, nothing is read or written out of bounds, and the image is then unspecified.  1 <= n_spans < 2^30; a NULL
 *   pointer or a size outside these ranges: TAN_ERR_BAD_ARG, nothing launched.
 * tan_rank_topk_filtered / _e4m3: tan_rank_topk / _e4m3 without pair, higher and ties, over the admitted rows only; 1 <= k <= 32,
 *   k <= N.  tan_rank_topk_video_filtered / _e4m3: tan_rank_topk_video / _e4m3 the same way: a video's entry is its best ADMITTED
 *   row, a video without an admitted row never appears.
 *   Result: the lists equal, bit for bit, the plain entry point's lists over the index made by gathering the admitted rows in
 *     order -- a score does not depend on where its row sits in a tile, a split or an index -- with top_row the row in THIS index
 *     and top_video the video of THIS v_off; equal scores by ascending row.  When fewer than k rows / videos are admitted the tail
 *     holds empty slots (-inf, row 0x7fffffff, video -1), which tan_topk_fold sorts last.  A filter that admits every row gives
 *     exactly the plain entry point's lists.
 *   A split walks a contiguous range of the image's tile list and streams only those tiles: the sweep's work follows the listed
 *     tiles, not N.  n_listed is read on the device: the grid is sized from (Q, N, splits) as for the plain call, and a workgroup
 *     whose range is empty writes empty lists and leaves.  The result does not depend on `splits`; no float atomics.
 *   filt: an image built for the same N (16-byte aligned).  An image of another N or a damaged one is the CALLER's error: list
 *     positions and tile numbers are clamped, nothing is read or written out of bounds, and the lists are unspecified.
 *   ws: tan_rank_topk_ws_bytes(Q, N, k) / tan_rank_topk_video_ws_bytes(Q, N, n_videos, k) bytes, as for the plain calls.
 *   Argument rules otherwise as tan_rank_topk / tan_rank_topk_video; k == 0 or a NULL filt: TAN_ERR_BAD_ARG, nothing launched.  */
long tan_row_filter_bytes(long N);
int tan_row_filter_build(const int* spans, long n_spans, long N, void* filt, void* stream);
int tan_rank_topk_filtered(const void* Tq, const void* Vn, int dtype, long Q, long N, int C, const void* filt, int k, int splits,
                           float* top_score, int* top_row, void* ws, void* stream);
int tan_rank_topk_filtered_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Q, long N, int C,
                                const void* filt, int k, int splits, float* top_score, int* top_row, void* ws, void* stream);
int tan_rank_topk_video_filtered(const void* Tq, const void* Vn, int dtype, long Q, long N, int C, const int* v_off, long n_videos,
                                 const void* filt, int k, int splits, float* top_score, int* top_row, int* top_video, void* ws,
                                 void* stream);
int tan_rank_topk_video_filtered_e4m3(const void* Tq, const float* q_scale, const void* Vn, const float* v_scale, long Q, long N,
                                      int C, const int* v_off, long n_videos, const void* filt, int k, int splits, float* top_score,
                                      int* top_row, int* top_video, void* ws, void* stream);

/* ---- corpus annotation: which of a fixed vocabulary of labels does every row of the index show (`search.annotate`) ----
 * tan_label_topk: the k best labels of every index row.  Tl [L, 512] label features, Vn [N, 512] index rows, in the formats of
 *   tan_rank_topk (TAN_F32: exact-f32 MFMA; TAN_BF16), 16-byte aligned.  top_score / top_label [N, k]: row n's k best
 *   (score f32, label int32) by descending score, equal scores by ascending label; score(l, n) is the f32 accumulation of the
 *   operand products, by the MFMA chain of tan_rank_topk(Tq = Tl, Vn).  1 <= k <= min(32, L), 1 <= L < 2^31, 1 <= N < 2^31.
 *   One launch, one workgroup per 128 index rows: the rows stay in registers (each is read from memory once in the whole launch),
 *   the labels stream through LDS in 64-label tiles, and a row's list is complete inside its workgroup -- nothing whose size
 *   grows with N * L is stored, no scratch, no merge launch, no atomics: bit-identical from run to run.  Tails in N and L are
 *   masked in the kernel.  Another width, k out of range, an unknown dtype, a NULL pointer, bad sizes: TAN_ERR_BAD_ARG, nothing
 *   launched.
 * tan_label_topk_e4m3: the same over the e4m3 codes and per-row power-of-two scales of tan_rank_topk_e4m3 (l_scale [L],
 *   v_scale [N]); score(l, n) = (acc * v_scale[n]) * l_scale[l], two f32 multiplies in that order -- tan_rank_topk_e4m3's formula
 *   with the label in the query's place.
 * tan_label_runs: the rows' best labels -> label segments.  lab[n] = top_label[n * stride] if top_score[n * stride] >= threshold,
 *   else -1 (background; a NaN score is background).  Only column 0 of the [N, stride] lists is read.  v_off [n_videos + 1] as in
 *   tan_rank_topk_video.  A RUN is a maximal range of rows [a, b] inside one video with lab constant and not -1 (two adjacent
 *   videos that end and begin with the same label give two runs); runs shorter than min_len (>= 1) are dropped.  The kept runs
 *   are written in ascending a: run_video, run_start = a, run_end = b (inclusive), run_label, run_peak_score = the largest
 *   top_score[n * stride] of the run and run_peak_row = the smallest row that attains it.  n_runs[0] = the number of kept runs,
 *   even above cap; only the first cap are written.  label_rows [L], if not NULL, is overwritten with the number of rows whose
 *   lab is l, whatever min_len is (integer atomics).  ws: tan_label_runs_ws_bytes(N) bytes (-1 for N outside [1, 2^31)), 4-byte
 *   aligned.  Six launches (flags / scan / fill / keep / scan / emit) and a memset of label_rows; every result is
 *   order-independent or computed in a fixed order: bit-identical from run to run.  A label outside [0, L) or a v_off that breaks
 *   its contract is the CALLER's error: labels and positions are clamped, nothing is read or written out of bounds, and the runs
 *   are then unspecified.  threshold NaN, min_len < 1, cap < 0, stride < 1, n_videos outside [1, N], a NULL pointer other than
 *   label_rows, sizes outside the ranges above: TAN_ERR_BAD_ARG, nothing launched.                                               */
int tan_label_topk(const void* Tl, const void* Vn, int dtype, long L, long N, int C, int k, float* top_score, int* top_label,
                   void* stream);
int tan_label_topk_e4m3(const void* Tl, const float* l_scale, const void* Vn, const float* v_scale, long L, long N, int C, int k,
                        float* top_score, int* top_label, void* stream);
long tan_label_runs_ws_bytes(long N);
int tan_label_runs(const float* top_score, const int* top_label, int stride, long N, long L, const int* v_off, long n_videos,
                   float threshold, int min_len, long cap, int* n_runs, int* run_video, int* run_start, int* run_end, int* run_label,
                   int* run_peak_row, float* run_peak_score, int* label_rows, void* ws, void* stream);

/* ---- temporally consistent labels: a per-video Viterbi decode over tan_label_topk's lists (`Annotation.decode`) ----
 * tan_label_decode: top_score f32 / top_label int32 [N, k] as tan_label_topk writes them, 1 <= k <= 32, 1 <= N < 2^31; v_off
 *   [n_videos + 1] as in tan_label_runs; threshold finite; switch_penalty in [0, +inf], not NaN.
 *   STATES of row t: j = 0 .. k-1 is list position j, with lab(t, j) = top_label[t, j] and gain(t, j) = top_score[t, j] - threshold
 *   (one f32 subtract), or -inf if the score is not finite (NaN, +-inf); state k is BACKGROUND, lab = -1 and gain = 0.
 *   OBJECTIVE, per video: over the paths s_t, maximise  sum_t gain(t, s_t) - switch_penalty * #{t >= 1 : lab(t, s_t) != lab(t-1,
 *   s_{t-1})}.  Staying on a label across a second where it scores below the threshold costs that second's negative gain; leaving
 *   and coming back costs two penalties.  A label that is not in a row's list is NOT AVAILABLE at that row -- a path cannot stay
 *   on it there -- so decode lists of k >= 5: with k = 1 only the best label or background can be chosen and nothing is bridged
 *   through a second whose best label is another one.
 *   ARITHMETIC, in this order, every operation one f32 add, subtract, max or compare (nothing to contract), so the result is
 *   defined bit for bit:   d[0][j] = gain(0, j).   For t >= 1:  m = max_i d[t-1][i],  a = the smallest i attaining it,
 *   rel[i] = d[t-1][i] - m;  for state j, i* = the smallest i with lab(t-1, i) == lab(t, j) (background always has one: k);
 *   if i* exists and rel[i*] >= -switch_penalty:  c = rel[i*], bp[t][j] = i*;  otherwise  c = -switch_penalty, bp[t][j] = a;
 *   d[t][j] = c + gain(t, j).   Subtracting m every step keeps d within a few units of 0 whatever the video's length.  The last
 *   row's state is the smallest j attaining max_j d; the walk back follows bp.  Videos do not interact.
 *   OUTPUTS: dec_label int32 [N]: the chosen state's label, -1 for background; dec_score f32 [N]: the chosen list entry's
 *   top_score, -inf for background.  A bridged second keeps its label with its own score, which is below the threshold.
 *   ws: tan_label_decode_ws_bytes(N, k) bytes -- N * (k + 1) back-pointer bytes plus alignment; any alignment of ws -- (-1 for
 *   sizes outside 1 <= N < 2^31, 1 <= k <= 32).  One launch: one wave per video (four per workgroup), sequential in time inside
 *   a video, so ONE very long video is one wave's serial chain -- the launch takes as long as its longest video.  No atomics:
 *   bit-identical from run to run and independent of the launch geometry.  Duplicate labels inside one row's list, or a v_off
 *   that breaks its contract, are the CALLER's error: indices are clamped, nothing is read or written out of bounds, and the
 *   result is then unspecified (so it is for gains that overflow f32).  A NULL pointer, k or sizes out of range, n_videos outside
 *   [1, N], a threshold that is not finite, a NaN or negative penalty: TAN_ERR_BAD_ARG, nothing launched.                         */
long tan_label_decode_ws_bytes(long N, int k);
int tan_label_decode(const float* top_score, const int* top_label, int k, long N, const int* v_off, long n_videos, float threshold,
                     float switch_penalty, int* dec_label, float* dec_score, void* ws, void* stream);

/* ---- copy alignment: the best local alignment of a query's seconds with a video's, re-timed or re-cut (`search.align_spans`) ----
 * A BLOCK is a row-major [m, V] f32 matrix of scores x[i][j], query second i along the rows, video second j along the columns:
 * what tan_sequence_scores writes for one hit (a query of more than 32 seconds as consecutive 32-row sequences with consecutive
 * x_off: a score does not depend on its tile position or query column).  With theta finite, skew in [0, +inf) and
 * H[-1][*] = H[*][-1] = 0:
 *     g[i][j] = x[i][j] - theta
 *     diag = H[i-1][j-1];   up = H[i-1][j] - skew;   left = H[i][j-1] - skew
 *     P    = max(diag, up, left);   pred = the FIRST of (diag, up, left) that attains P
 *     H[i][j] = max(0, g[i][j] + P)
 * Every - and + is one f32 operation, round to nearest, never contracted; every max is exact.  Each cell is therefore a fixed
 * function of three neighbours: given the bits of x, the result does not depend on traversal order, strip height, slab width or
 * launch shape.  For a cell with H > 0: if pred is diag and that H is 0 (or lies outside the matrix) the path STARTS here, origin =
 * (i, j), cells = 1; otherwise origin and cells + 1 are inherited from pred (an up or left that attains P ahead of diag has H > 0).
 * Per block: best = max H; end = the cell attaining best with the smallest i, then the smallest j; score = best and span =
 * (a_first, a_last, b_first, b_last, cells) = (origin i, end i, origin j, end j, the end's cells): query seconds a_first .. a_last
 * shown as video seconds b_first .. b_last.  No positive cell: score = 0, span = (-1, -1, -1, -1, 0).  Inputs are finite.
 * This is Smith-Waterman in its time-warping form: horizontal and vertical steps are matches too (one query second shown for two
 * video seconds, or the reverse) and cost skew; an unrelated cell costs theta - x, so a short cut or insertion is bridged and a long
 * one is not.  tan_sequence_topk / tan_monotonic_decode are global and one-sided; tan_clip_topk is a diagonal of slope one.
 * tan_local_align: x holds n_x elements; x_off [P] `long` element offsets and table [P, 3] int32 = (m, V, first boundary slot) on
 *   the device, the slot being the running sum of V over the entries before (slots of different entries must not overlap), sum_V
 *   the sum over all.  1 <= m <= 4096, 1 <= V < 2^20, m * V < 2^31; score f32 [P], span int32 [P, 5].
 *   ws: tan_local_align_ws_bytes(P, sum_V) bytes, any alignment: two boundary rows of 16 bytes per slot (the last row of a strip of
 *   64 query seconds, handed to the next strip), 32 * sum_V + 16; -1 for P or sum_V outside [1, 2^31) or sum_V < P.
 *   One launch: one wave per block (four per workgroup), the strips of a block one after the other, the anti-diagonals of a strip
 *   in sequence -- so ONE long pair is one wave's serial chain of about (m / 64) * (V + 63) steps.  No atomics: bit-identical from run
 *   to run.  A NULL pointer, n_x < 1, P or sum_V out of range, a theta that is not finite, a skew that is negative, infinite or NaN:
 *   TAN_ERR_BAD_ARG, nothing launched.  A table entry outside the limits, whose block leaves [0, n_x) or whose slots leave
 *   [0, sum_V) is skipped with the empty result, as tan_sequence_scores skips a bad hit; nothing is read or written out of bounds. */
long tan_local_align_ws_bytes(long P, long sum_V);
int tan_local_align(const float* x, long n_x, const long* x_off, const int* table, long P, long sum_V, float theta, float skew,
                    float* score, int* span, void* ws, void* stream);

/* ---- copy alignment with the path: the second-to-second time map of the best local alignment (`search.align_paths`) ----
 * This ADDS to tan_local_align's definition and changes nothing in it.  Each positive cell gets one 2-bit CODE:
 *     0 start: pred is diag and that H is 0 or lies outside the matrix;   1 diag;   2 up;   3 left
 * with pred the first of (diag, up, left) attaining P, as above.  The PATH of a block with score > 0 is the chain of cells from
 * `end` back along the codes to its start cell.  It has exactly `cells` cells and is monotone in i and j, so the cells of query
 * second i are consecutive video seconds lo_i .. hi_i, and lo_{i+1} is hi_i or hi_i + 1.  The TIME MAP qmap is int32 [m, 2] per
 * block: row i = (lo_i, hi_i) for a_first <= i <= a_last, (-1, -1) in every other row and in all rows of a block without a
 * positive cell.  Hence qmap[a_first][0] == b_first, qmap[a_last][1] == b_last, sum (hi - lo + 1) == cells, and the map is a
 * fixed function of the bits of x whatever the launch shape.
 * tan_local_align_path: x, n_x, x_off, table, P, sum_V, theta, skew, score, span as for tan_local_align; score and span are
 *   tan_local_align's bit for bit.  path_off [P, 2] `long` on the device: column 0 the first qmap row of each block -- the running
 *   sum of m; the block owns m rows of qmap int32 [n_map, 2] --, column 1 its first TRACE entry -- the running sum of
 *   ceil(m / 64) * (V + 63), n_trace the total.  The trace is one 16-byte entry per (strip of 64 query seconds, anti-diagonal d):
 *   two 64-bit masks, the low and the high bit of the code of cell (i, j) at bit i & 63 of entry (i >> 6, j + (i & 63)).
 *   ws: tan_local_align_path_ws_bytes(P, sum_V, n_trace) = 32 * sum_V + 16 * n_trace + 16 bytes, any alignment (-1 for P or sum_V as
 *   above, n_trace outside [1, 2^35)).  One launch, one wave per block as tan_local_align; the same wave walks the path back
 *   (about (m + V) / 32 dependent loads of 1 KiB) and writes the block's m map rows.  No atomics: bit-identical from run to run.
 *   An entry is skipped if tan_local_align would skip it, or if its map rows leave [0, n_map) or its trace entries leave
 *   [0, n_trace): the empty score and span, and NOTHING of qmap is touched.  A valid entry writes all m of its map rows: the caller
 *   never clears qmap.  TAN_ERR_BAD_ARG, nothing launched: tan_local_align's cases, a NULL path_off or qmap, n_map outside
 *   [1, 2^31), n_trace outside [1, 2^35).                                                                                      */
long tan_local_align_path_ws_bytes(long P, long sum_V, long n_trace);
int tan_local_align_path(const float* x, long n_x, const long* x_off, const int* table, long P, long sum_V, float theta, float skew,
                         const long* path_off, long n_map, long n_trace, float* score, int* span, int* qmap, void* ws, void* stream);

/* ---- step discovery: the update half of spherical k-means over the index's rows (`search.discover_steps`) ----
 * The assignment half is tan_label_topk / _e4m3 with the centroids as the labels and k = 1.
 * tan_cluster_accumulate: Vn [N, 512] index rows in the formats of tan_label_topk (TAN_F32, TAN_BF16; 16-byte aligned), assign
 *   int32 [N]: every row's cluster, order int32 [N]: a permutation of the rows, sums [K, 512] `long` (64-bit, 8-byte aligned).
 *   With v the element as f32 (bf16 widened) and q(n, j) = (long) round-to-nearest-even(v * 2^30) -- the f32 multiply by a power
 *   of two is exact, the conversion is __float2ll_rn --:
 *       sums[assign[n]][j] += q(n, j)      for every row n, in wrapping 64-bit integer arithmetic.
 *   The kernel ADDS: the caller zeroes sums once, and several launches (one per shard of an index) add into the same buffer.
 *   Integer addition is associative, so the result is the same bits for EVERY permutation `order`, for any split of the rows over
 *   launches and from run to run, although the flushes are atomics.  `order` only decides how many atomics are issued: a wave
 *   walks tan_cluster_slab_rows() = 256 consecutive positions of it and flushes its registers when the cluster changes, so with
 *   order sorted by cluster a launch issues at most (N / 256 + K) * 512 64-bit atomics -- 16 bytes per row and 4 KiB per cluster,
 *   against the 1 KiB (bf16) it reads per row.
 *   Contract: |v| <= 2 (index rows are unit vectors), so fewer than 2^31 rows cannot overflow a sum; the image q is exact for every
 *   bf16 value of magnitude >= 2^-23.  A row whose assign lies outside [0, K), or a position whose order lies outside [0, N), is
 *   skipped.  A non-finite v contributes an unspecified value; nothing is read or written out of bounds whatever assign and order
 *   hold.  1 <= N < 2^31, 1 <= K < 2^31; another width than 512, an unknown dtype, a NULL pointer, bad sizes or alignment:
 *   TAN_ERR_BAD_ARG, nothing launched.
 * tan_cluster_accumulate_e4m3: the same over the e4m3 codes and per-row power-of-two scales of tan_rank_topk_e4m3 (v_scale [N]);
 *   v = decode(code) * v_scale[n], one f32 multiply.
 * tan_cluster_centroids: sums [K, 512] as above, counts int32 [K]: the rows of every cluster, prev f32 [K, 512] -> cent f32
 *   [K, 512], cohesion f32 [K].  One wave per cluster; every step is ONE correctly rounded f32 operation, never contracted:
 *       x_j    = (float) sums[c][j] * 2^-30            (int64 -> f32 round to nearest even; the scaling is exact)
 *       norm2  : lane l = 0 .. 63 adds x_j * x_j over j = l, l + 64, ..., l + 448 in that order (to 0), then the 64 partial sums
 *                are folded by an xor butterfly over the lane distances 32, 16, 8, 4, 2, 1: p[l] = p[l] + p[l ^ d]
 *       norm   = sqrt(norm2);   cent[c][j] = x_j / norm  (a division, not a reciprocal);   cohesion[c] = norm / (float) counts[c]
 *   cohesion is the mean resultant length of the cluster's rows, in [0, 1] for unit rows: 1 when they all coincide.  If
 *   counts[c] <= 0, or norm is 0 or not finite: cent[c] = prev[c] bit for bit and cohesion[c] = 0 -- an empty cluster keeps its
 *   centroid.  cent may be prev itself.  1 <= K < 2^31; another width, a NULL pointer: TAN_ERR_BAD_ARG, nothing launched.        */
int tan_cluster_slab_rows(void);
int tan_cluster_accumulate(const void* Vn, int dtype, long N, int C, const int* assign, const int* order, long K, long* sums,
                           void* stream);
int tan_cluster_accumulate_e4m3(const void* Vn, const float* v_scale, long N, int C, const int* assign, const int* order, long K,
                                long* sums, void* stream);
int tan_cluster_centroids(const long* sums, const int* counts, const float* prev, long K, int C, float* cent, float* cohesion,
                          void* stream);

/* ---- storyboards: the k seconds that together show a video best (`search.storyboard`) ----
 * A video has rows r_0 .. r_{V-1}.  x[s][t] is the row sweep's score with row s as the QUERY row and row t as the index row: the bits
 * tan_sequence_scores writes for the video's own rows, cut into 32-row pieces, against the video -- one row-major [V, V] block (e4m3:
 * (acc * v_scale[t]) * q_scale[s], the row's own scale on both sides).  x[s][t] == x[t][s] is NOT assumed.  Greedy facility location:
 *     fix(x)  = __float2ll_rn(x * 2^30f)                                    (tan_cover_topk's image; the multiply is exact)
 *     C_0[t]  = -2^62 for every t
 *     T_j(s)  = sum_t max(fix(x[s][t]), C_{j-1}[t])                         (64-bit integers: order-free)
 *     s_j     = the s with the largest T_j(s); equal sums: the lowest s
 *     stop before writing entry j (j >= 2) when
 *             gain = T_j(s_j) - sum_t C_{j-1}[t] <= 0
 *          or gain < G_min * V,   G_min = min(__float2ll_rn(min_gain * 2^30f), 2^40)
 *     C_j[t]  = max(C_{j-1}[t], fix(x[s_j][t]))
 *     owner[t] = j wherever fix(x[s_j][t]) > C_{j-1}[t] (strictly), else kept
 *     coverage[j] = ((float) sum_t C_j[t] * 2^-30f) / (float) V             (int64 -> f32 round to nearest even, exact scaling, ONE f32 division)
 * Contract: |x| <= 2 and finite (index rows are unit vectors), so no sum overflows; a gain is then below 2^32 * V, which is why the
 * clamp of G_min changes nothing and G_min * V is exact.  The entries are stored 0-BASED: second[j - 1] = s_j as a second of the
 * video (0 = its first), coverage[j - 1], and owner[t] = j - 1.  The first entry is always made (the row with the largest summed
 * score; every owner is then 0); a row already chosen has gain 0, so no second is chosen twice.  Entries after a stop, and entries
 * beyond V, hold second = -1 and coverage = 0.  coverage is the mean over the video's seconds of the best score to any second chosen
 * so far: it does not decrease.  owner[t] is the entry that shows second t best, equal scores going to the earliest entry.  Every
 * sum is an integer: given the bits of x the result depends on no reduction order, tiling or launch shape.
 * tan_storyboard_select: x holds n_x elements; x_off [P] `long` element offsets and table [P, 2] int32 = (V, first owner slot) on the
 *   device, the slot being the running sum of V over the entries before, sum_V the sum over all (tan_local_align's layout with m = V).
 *   second int32 [P, k], coverage f32 [P, k]: always fully written; owner int32 [sum_V].  1 <= V <= 4096
 *   (tan_storyboard_max_rows()), 1 <= k <= 4096, min_gain finite and >= 0.
 *   One launch, one workgroup per video, which runs the k iterations itself: C in LDS (32 KiB), every candidate row read once per
 *   iteration, a wave per row; no scratch, no atomics, bit-identical from run to run.  A video costs min(k, V) * V * V score reads:
 *   V and k near their limits TOGETHER are one workgroup's serial chain of minutes.
 *   A NULL pointer, n_x < 1, P or sum_V outside [1, 2^31), sum_V < P, k outside [1, 4096], a min_gain that is negative, infinite or
 *   NaN: TAN_ERR_BAD_ARG, nothing launched, nothing written.  A table entry outside the limits, whose block leaves [0, n_x) or whose
 *   slots leave [0, sum_V), gets the empty result (second = -1, coverage = 0) and its owner slots are NOT written; every other entry
 *   is computed, and nothing is read or written out of bounds -- tan_local_align's convention.                                      */
int tan_storyboard_max_rows(void);                 /* 4096 */
int tan_storyboard_select(const float* x, long n_x, const long* x_off, const int* table, long P, long sum_V, int k, float min_gain,
                          int* second, float* coverage, int* owner, void* stream);

/* ---- chapters: a video cut into contiguous scenes by an exact dynamic programme (`search.chapters`) ----
 * Kernel temporal segmentation (Potapov et al., ECCV 2014) over a video's own block.  x[s][t] is the video's block exactly as
 * storyboards define it above: the bits tan_sequence_scores writes.  x[s][t] == x[t][s] is NOT assumed; only sums over squares are
 * used.  fix(x) = __float2ll_rn(x * 2^30f).  All arithmetic below is on 64-bit integers.  INF = 2^62.
 * Costs, for 0 <= s < e <= V:
 *     D(s,e) = sum_{s<=t<e} fix(x[t][t])
 *     Q(s,e) = sum_{s<=i<e} sum_{s<=t<e} fix(x[i][t])
 *     J(s,e) = D(s,e) - floor(Q(s,e) / (e - s))                            floor toward minus infinity
 * Decode, with the parameters k, min_len >= 1 and penalty >= 0, and m = min(k, V):
 *     G       = min(__float2ll_rn(penalty * 2^30f), 2^50)
 *     dp_1[e] = J(0,e) if e >= min_len or e == V, else INF                  (a video shorter than min_len is one chapter)
 *     dp_j[e] = min over s in [1, e - min_len] with dp_{j-1}[s] < INF of dp_{j-1}[s] + J(s,e)             (2 <= j <= m)
 *               equal sums: the LOWEST s, kept as arg_j[e]; INF if there is no such s
 *     j is feasible when dp_j[V] < INF (j = 1 always is)
 *     count   = the lowest feasible j with the smallest dp_j[V] + (j - 1) * G
 *     b_count = V;  b_{j-1} = arg_j[b_j]
 *     start[c] = b_c for c = 0 .. count-1                                   (start[0] = 0)
 *     chapter[t] = c for start[c] <= t < start[c+1]
 *     scatter[j-1] = (float) dp_j[V] * 2^-30f                               (one int64 -> f32 rounding, exact scaling)
 * scatter[j-1] is the f32 +infinity (bits 0x7f800000) for every infeasible j <= k; start[c] = -1 for c >= count.  penalty is
 * absolute, in score x seconds: a boundary is kept only if it lowers the summed scatter by at least that much (merging two scenes of
 * a and b seconds costs about ab / (a + b) times their squared distance, whatever the video's length).
 * Contract: |x| <= 2 and finite.  Then |Q| <= 2^55, |J| < 2^45, every dp stays below 2^46 and (j - 1) * G < 2^58.
 * x_off [P] `long` element offsets and table [P, 2] int32 = (V, first chapter slot) are tan_storyboard_select's tables.
 * tan_chapter_costs: cost holds n_x 64-bit elements at the same element offsets as x: cost[x_off[p] + (e-1)*V + s] = J(s,e) for
 *   0 <= s < e <= V.  The other half of a video's block is the kernels' to use; its contents are unspecified afterwards.  Nothing
 *   outside a video's block is written.  Three launches over all videos of the call (row scans, the upper triangle's column scans,
 *   the lower triangle's column scans with the transposed upper tile through LDS and the division), all in place in cost; the
 *   column scans walk 64 x 64 tiles with carries.  No scratch, no atomics, no allocation; bit-identical from run to run.
 *   A NULL pointer, n_x < 1, P outside [1, 2^31): TAN_ERR_BAD_ARG, nothing launched.  A table entry with V outside [1, 4096]
 *   (tan_chapter_max_rows()) or whose block leaves [0, n_x) is skipped: its cost block stays untouched (the slot column is not read).
 * tan_chapter_decode: count int32 [P], start int32 [P, k], scatter f32 [P, k]: always fully written; chapter int32 [sum_V].
 *   1 <= V <= 4096, 1 <= k <= 256, 1 <= min_len <= 4096, penalty finite and >= 0.  ws: tan_chapter_decode_ws_bytes(P, sum_V, k)
 *   bytes (sum_V * k * 2: arg_j[e] as 16 bits; TAN_ERR_BAD_ARG for sizes the entry point refuses), caller-owned.
 *   One launch, one workgroup of 16 waves per video, which runs every level itself: dp_{j-1} and dp_j in LDS (2 x 4097 x 8 bytes), a
 *   wave per end e reads row e - 1 of the costs from column (j-1) * min_len to e - min_len in 16-byte loads and keeps its next
 *   row's first loads in flight across the reduction; ends below j * min_len are INF without a read; the levels stop at
 *   min(k, V / min_len).  No scratch, no atomics, bit-identical from run to run.  A video reads about min(k, V / min_len) * V^2 / 2
 *   cost elements of 8 bytes through ONE workgroup: V and k near their limits TOGETHER are a serial chain of minutes.
 *   A NULL pointer, n_x < 1, P or sum_V outside [1, 2^31), sum_V < P, k outside [1, 256], min_len outside [1, 4096], a penalty that
 *   is negative, infinite or NaN: TAN_ERR_BAD_ARG, nothing launched, nothing written.  A table entry outside the limits, whose block
 *   leaves [0, n_x) or whose slots leave [0, sum_V), gets the empty result (count = 0, start = -1, scatter = +inf) and its chapter
 *   slots are NOT written; every other entry is computed, and nothing is read or written out of bounds.                            */
int tan_chapter_max_rows(void);                    /* 4096 */
int tan_chapter_costs(const float* x, long n_x, const long* x_off, const int* table, long P, long* cost, void* stream);
long tan_chapter_decode_ws_bytes(long P, long sum_V, int k);
int tan_chapter_decode(const long* cost, long n_x, const long* x_off, const int* table, long P, long sum_V, int k, int min_len,
                       float penalty, int* count, int* start, float* scatter, int* chapter, void* ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TAN_HIP_H */

/*
 * dic_hip.h -- C ABI of the MI355X (gfx950) hot path of deep-interpolation-clustering.
 *
 * One shared object (libdic_hip.so), extern "C", plain pointers and sizes only.
 * Conventions shared by every compute entry point:
 *   - returns DIC_OK (0) or a negative dic_status code; never throws, never allocates;
 *   - every pointer is a DEVICE pointer owned by the caller and borrowed for the call;
 *   - work is enqueued asynchronously on `stream` (a hipStream_t passed as void*);
 *   - `workspace` buffers are caller-allocated scratch; query their size first;
 *   - kernels hold no global mutable state and are re-entrant across streams.
 *
 * The reference has no FFI: its boundary is the Python module surface.  Each entry
 * point below names the reference lines (relative to the upstream repository) whose
 * arithmetic it replaces; INTEGRATION.md shows the ctypes stub that binds them
 * behind the upstream module names.
 *
 * Stacked input layout (reference: interpolation_layer.py:25-30, dataloader.py:54-69):
 *   x is (B, 4C, T) contiguous f32; planes [value*mask | mask | time(h) | hold-out].
 *   `lengths` (B,C) int32 is optional: when given, row (b,c) is a PREFIX of
 *   lengths[b,c] valid slots (what p0/the trainers always produce) and the mask
 *   plane is not read; when NULL the mask plane is honoured slot by slot.
 * Packed ragged layout (dataset-resident fast path):
 *   row_off (B*C+1) int64 offsets into packed `t_pk`/`v_pk` f32 arrays, rows stored
 *   back to back in (b,c) order; max_len = longest row.
 */
#ifndef DIC_HIP_H
#define DIC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIC_ABI_VERSION 1

typedef enum dic_status {
    DIC_OK = 0,
    DIC_ERR_INVALID_ARG = -1,   /* NULL pointer, non-positive size                      */
    DIC_ERR_UNSUPPORTED = -2,   /* shape outside the compiled limits (see each entry)   */
    DIC_ERR_WORKSPACE = -3,     /* workspace too small                                  */
    DIC_ERR_LAUNCH = -4         /* hipGetLastError() != hipSuccess after the launch     */
} dic_status;

typedef void* dic_stream_t;    /* hipStream_t */

/* Limits compiled into the kernels. */
#define DIC_MAX_CHANNELS 16    /* C  (C*C <= one 256-thread workgroup) */
#define DIC_MAX_REFPOINTS 64   /* R  */
#define DIC_MAX_CLUSTERS 32    /* K  */
#define DIC_LATENT_MAX_DIM 256 /* D: latent rows are handled 4 columns per lane by one wave */

int dic_version(void);
const char* dic_status_string(int status);
const char* dic_last_error_string(void);   /* detail of the last failure on this thread */

/* ------------------------------------------------------------------ k1: SCI (+CCI) ------
 * Replaces SingleChannelInterp.forward (interpolation_layer.py:31-86) and, when
 * cci_kernel != NULL, CrossChannelInterp.forward fused as its epilogue
 * (interpolation_layer.py:99-127).
 *   out   (B,R,3C): cci_kernel==NULL -> [y | w | y_trans]; else [smooth | exp(w) | y_trans-smooth]
 *   saved (B,7,C,R) or NULL: y,w,y_trans,Eu1,Exu1,Eu10,Exu10 -- what the backward needs
 *          (Eu = E_s[u], Exu = E_s[x u] under the softmax weights, u=(t-ref)^2).
 * A channel with no valid observation yields NaN y/y_trans and w=-inf, as upstream.
 * ref_grid (R) f32 = the reference time grid, i.e. torch.linspace(0, hours, R) (interpolation_layer.py:41),
 * passed as data so the kernel sees bit-identical grid values.
 * Limits: C<=16, R<=64, one encounter (2*C*T f32 + results) must fit 64 KB of LDS. */
int dic_sci_cci_fwd(const float* x, const int32_t* lengths, int B, int C, int T, int R, const float* ref_grid,
                    const float* sci_kernel, const float* cci_kernel,
                    float* out, float* saved, dic_stream_t stream);

int dic_sci_cci_fwd_ragged(const float* t_pk, const float* v_pk, const int64_t* row_off, int max_len,
                           int B, int C, int R, const float* ref_grid,
                           const float* sci_kernel, const float* cci_kernel,
                           float* out, float* saved, dic_stream_t stream);

/* The same forward reading a RAGGED ENCOUNTER STORE in place (the device-resident form of the feed_data array
 * dataloader.py:54-79 builds): for every (encounter, channel) row only the observed samples, packed back to back --
 *   t_pk, v_pk   packed time stamps (h) and values (ob * mask, rescaled): row g of the store at [row_off[g], row_off[g+1]);
 *   hold_pk      optional packed hold-out flags (plane 3, p0_data_process.py:95-117): the model input is v * hold (a denoising
 *                step, pretrain_trainer.py:139-141);
 *   row_off      (N*C + 1) int64; the packed arrays must keep >= 64 readable elements behind the last row;
 *   enc_idx      (B) int32 store encounter of each batch row (a shuffled batch is read in place: no gather, no padded copy), or
 *                NULL: the batch is encounters 0..B-1;
 *   lengths      (B,C) int32 row lengths of the BATCH rows (= the store's, gathered), or NULL: taken from row_off;
 *   T            the padded width the dense path would have (bounds every row; sizes the LDS rows).
 * times_sorted != 0: the caller certifies that every row's time stamps are non-decreasing (ragged.RaggedStore checks it once when the cohort is packed):
 * the soft-max shift min_t (t - ref)^2 is then found by bisection instead of a pass over the row -- the same value, bit for bit.
 * out (B,R,3C) f32 and / or xenc (R,B,xw) bf16 packed rows as dic_sci_cci_fwd_packed; saved as above.  Same arithmetic, same results
 * as the dense entry points on the same samples. */
int dic_sci_cci_fwd_store(const float* t_pk, const float* v_pk, const uint8_t* hold_pk, const int64_t* row_off, const int32_t* enc_idx,
                          const int32_t* lengths, int B, int C, int T, int R, const float* ref_grid, const float* sci_kernel,
                          const float* cci_kernel, float* out, float* saved, void* xenc, int xw, int times_sorted, dic_stream_t stream);

/* Backward of the above wrt the two parameters only (the inputs carry no gradient upstream).
 *   grad_out (B,R,3C) cotangent of `out`; saved from the forward;
 *   grad_sci_kernel (C), grad_cci_kernel (C,C; ignored when cci_kernel==NULL): OVERWRITTEN.
 * Deterministic two-stage reduction through `workspace`. */
size_t dic_sci_cci_bwd_workspace(int B, int C, int R);
int dic_sci_cci_bwd(const float* grad_out, const float* saved, const float* sci_kernel,
                    const float* cci_kernel, int B, int C, int R,
                    float* grad_sci_kernel, float* grad_cci_kernel,
                    void* workspace, size_t workspace_bytes, dic_stream_t stream);

/* Stand-alone CrossChannelInterp on an arbitrary (B,R,3C) tensor s=[y|w|y_trans]
 * (interpolation_layer.py:99-127) and its backward wrt both s and the kernel. */
int dic_cci_fwd(const float* s, const float* cci_kernel, int B, int C, int R, float* out,
                dic_stream_t stream);
size_t dic_cci_bwd_workspace(int B, int C, int R);
int dic_cci_bwd(const float* grad_out, const float* s, const float* cci_kernel, int B, int C, int R,
                float* grad_s, float* grad_cci_kernel,
                void* workspace, size_t workspace_bytes, dic_stream_t stream);

/* The fused pair feeding the encoder LSTM without a layout pass: the forward additionally (out may then be NULL) writes
 * xenc (R,B,xw) bf16 = rows [cci(sci(x)) (3C) | 1 | 0 ...] -- time-major, padded to the MFMA k-step, the constant one carrying
 * the LSTM bias (dic_lstm_fwd_proj) -- and the backward takes the encoder's input gradient in that same layout. */
int dic_sci_cci_fwd_packed(const float* x, const int32_t* lengths, int B, int C, int T, int R, const float* ref_grid,
                           const float* sci_kernel, const float* cci_kernel, float* out, float* saved, void* xenc, int xw,
                           dic_stream_t stream);
int dic_sci_cci_bwd_packed(const void* grad_packed, int xw, const float* saved, const float* sci_kernel, const float* cci_kernel,
                           int B, int C, int R, float* grad_sci_kernel, float* grad_cci_kernel, void* workspace,
                           size_t workspace_bytes, dic_stream_t stream);

/* ------------------------------------------------------------------ k2: RBF de-interpolation
 * Replaces RBF.forward minus compress_fc (rbf.py:57-108, gaussian rbf.py:129-131).
 *   v (B,C,R) = compress_fc output;  y (B,C,T) OVERWRITTEN (0 in masked slots).
 * Limits: C<=16, R<=64.  * v_time_major != 0: v (and grad_v) are laid out (R,B,C) -- the row order TimeDistributed(CompressFC) produces them in on the
 * decoder's (R,B,.) output -- instead of (B,C,R): no transposing copy between the FC head and this kernel.
  * norm (optional, saved for the backward) = 1 / (sum_r phi + 1e-10) per valid slot.  prefix_only != 0 (with lengths): only the first
 * n slots of each row of y / norm (dic_masked_sse_bwd: of grad_rec) are written -- the training step never reads the padding, which
 * is half of the 96-slot rows at ~50 observations per channel; with 0 the padding is written as zeros, as upstream's `* mask` does.
 */
int dic_rbf_fwd(const float* x, const int32_t* lengths, int B, int C, int T, int R, const float* ref_grid,
                const float* rbf_kernel, const float* v, int v_time_major, float* y, float* norm /* (B,C,T) or NULL: saved for the
                backward */, int prefix_only, dic_stream_t stream);

/* grad_y (B,C,T) -> grad_v (B,C,R), grad_rbf_kernel (C); both OVERWRITTEN.  y, norm: forward outputs.
 * Masks are binary upstream; a non-zero mask value is treated as 1. */
size_t dic_rbf_bwd_workspace(int B, int C, int T, int R);
int dic_rbf_bwd(const float* x, const int32_t* lengths, int B, int C, int T, int R, const float* ref_grid,
                const float* rbf_kernel, const float* v, int v_time_major, const float* y, const float* norm,
                const float* grad_y, float* grad_v, float* grad_rbf_kernel,
                void* workspace, size_t workspace_bytes, dic_stream_t stream);

/* k2 with the reconstruction loss riding along (RBF.forward + Net.rec_loss, rbf.py:57-108 + clustering_interp.py:197-203), for the
 * training step, where the reconstruction is consumed by the loss alone:
 *   dic_rbf_fwd_loss: as dic_rbf_fwd, and out2[0] = sum over the valid slots of (y - ob)^2, out2[1] = #valid slots (what
 *     dic_masked_sse_fwd returns for a binary mask) from the values the kernel holds in registers -- no second pass over y and ob;
 *   dic_rbf_bwd_loss: as dic_rbf_bwd with dL/dy = grad_loss[0] * 2 (y - ob) / sse_count[1] on the valid slots formed on the fly from ob
 *     (prefix masks: lengths required) -- the (B,C,T) gradient of the reconstruction is never written or read.
 * sse_count = out2 after the caller's all-reduce over ranks; grad_loss (1) = dL/d(out2[0] / out2[1]); all device pointers. */
size_t dic_rbf_fwd_loss_workspace(int B, int C, int T, int R);
int dic_rbf_fwd_loss(const float* x, const int32_t* lengths, int B, int C, int T, int R, const float* ref_grid, const float* rbf_kernel,
                     const float* v, int v_time_major, const float* ob, float* y, float* norm, int prefix_only, float* out2,
                     void* workspace, size_t workspace_bytes, dic_stream_t stream);
int dic_rbf_bwd_loss(const float* x, const int32_t* lengths, int B, int C, int T, int R, const float* ref_grid, const float* rbf_kernel,
                     const float* v, int v_time_major, const float* y, const float* norm, const float* ob, const float* sse_count,
                     const float* grad_loss, float* grad_v, float* grad_rbf_kernel, void* workspace, size_t workspace_bytes,
                     dic_stream_t stream);

/* k2 reading the ragged encounter store in place (see dic_sci_cci_fwd_store for t_pk / v_pk / row_off / enc_idx / lengths; lengths is
 * required here): the time stamps come from t_pk and -- for the fused reconstruction loss -- the observations from v_pk, so the
 * padded (B,4C,T) input and the (B,C,T) observation tensor do not exist on this path.  y, norm (and grad_y when given) stay (B,C,T).
 *   dic_rbf_fwd_store: with_loss != 0 = dic_rbf_fwd_loss (out2, workspace of dic_rbf_fwd_loss_workspace bytes), else dic_rbf_fwd;
 *   dic_rbf_bwd_store: grad_y == NULL = dic_rbf_bwd_loss (sse_count, grad_loss required), else dic_rbf_bwd. */
int dic_rbf_fwd_store(const float* t_pk, const float* v_pk, const int64_t* row_off, const int32_t* enc_idx, const int32_t* lengths,
                      int B, int C, int T, int R, const float* ref_grid, const float* rbf_kernel, const float* v, int v_time_major,
                      int with_loss, float* y, float* norm, int prefix_only, float* out2, void* workspace, size_t workspace_bytes,
                      dic_stream_t stream);
int dic_rbf_bwd_store(const float* t_pk, const float* v_pk, const int64_t* row_off, const int32_t* enc_idx, const int32_t* lengths,
                      int B, int C, int T, int R, const float* ref_grid, const float* rbf_kernel, const float* v, int v_time_major,
                      const float* y, const float* norm, const float* grad_y, const float* sse_count, const float* grad_loss,
                      float* grad_v, float* grad_rbf_kernel, void* workspace, size_t workspace_bytes, dic_stream_t stream);

/* Net.rec_loss (clustering_interp.py:197-203): out2[0]=sum((rec*m-ob*m)^2), out2[1]=#{m==1}.
 * mask (B,C,T) may be NULL when lengths is given.  The loss is out2[0]/out2[1]. */
size_t dic_masked_sse_workspace(int B, int C, int T);
int dic_masked_sse_fwd(const float* ob, const float* rec, const float* mask, const int32_t* lengths,
                       int B, int C, int T, float* out2,
                       void* workspace, size_t workspace_bytes, dic_stream_t stream);
/* grad_rec = grad_loss[0] * 2*m*(rec*m-ob*m)/sse_count[1]   (all device pointers). */
int dic_masked_sse_bwd(const float* ob, const float* rec, const float* mask, const int32_t* lengths,
                       int B, int C, int T, const float* sse_count, const float* grad_loss,
                       float* grad_rec, int prefix_only, dic_stream_t stream);

/* ------------------------------------------------------------------ k3: DEC ---------------
 * Replaces ClusterAssignment.forward (dec.py:49-63).
 *   z (B,D), centers (K,D) -> q (B,K); tsaved (B,K) or NULL = 1/(1+d2/alpha) for the backward;
 *   colsum (K) or NULL = sum_i q_ij (the batch-level f_j of dec.py:73; all-reduce it when sharded).
 * Limits: D%4==0, D<=256, K<=32. */
size_t dic_dec_fwd_workspace(int B, int D, int K);
int dic_dec_fwd(const float* z, const float* centers, int B, int D, int K, float alpha,
                float* q, float* tsaved, float* colsum,
                void* workspace, size_t workspace_bytes, dic_stream_t stream);
/* target_distribution (dec.py:66-76) given the (global) column sums. */
int dic_dec_target(const float* q, const float* colsum, int B, int K, float* p, dic_stream_t stream);
/* Backward of dic_dec_fwd: grad_q (B,K) -> grad_z (B,D), grad_centers (K,D); OVERWRITTEN. */
size_t dic_dec_bwd_workspace(int B, int D, int K);
int dic_dec_bwd(const float* z, const float* centers, const float* q, const float* tsaved,
                const float* grad_q, int B, int D, int K, float alpha,
                float* grad_z, float* grad_centers,
                void* workspace, size_t workspace_bytes, dic_stream_t stream);
/* Fused Net.kl_loss (clustering_interp.py:205-207) forward + d/dq:
 *   kl_out[0] = sum_ij p (log p - log q) / batch_div ; grad_q (B,K) or NULL = -gscale*p/(batch_div*q). */
size_t dic_dec_kl_workspace(int B, int K);
int dic_dec_kl(const float* q, const float* p, int B, int K, float batch_div, float gscale,
               float* kl_out, float* grad_q,
               void* workspace, size_t workspace_bytes, dic_stream_t stream);

/* ------------------------------------------------------------------ k4: k-means -----------
 * Replaces the Lloyd E+M step scikit-learn runs for KMeans.fit/predict at
 * clustering_trainer.py:75-82, p2_clustering_optK.py:260-389, p4_clustering_final.py:159-174
 * (sklearn 1.7.2 _k_means_lloyd.pyx:23-218, _k_means_common.pyx:167-311).
 * `n_runs` independent problems on the SAME data share one launch (restarts / n_init).
 *   X (N,D) f32 (already mean-centred by the caller, as sklearn does), xnorm (N) = ||x||^2,
 *   centers (n_runs,K,D) IN/OUT: replaced by the updated centres,
 *   labels  (n_runs,N) int32 IN/OUT: previous labels in (use -1 before the first call),
 *   status  (n_runs,DIC_KM_STATUS_WORDS) f32 IN/OUT, zero it before the first iteration:
 *     [0] done flag (1 = converged: this and later calls are no-ops for the run)
 *     [1] iterations executed   [2] last center_shift_tot   [3] last #labels changed
 *     [4] strict-convergence flag [5] relocations performed [6] tol (IN) [7] max_iter (IN)
 * One call = one Lloyd iteration for every run that is not done: assign by
 * argmin_j(||c_j||^2 - 2 x.c_j) (first minimum wins), accumulate sums/counts, relocate empty
 * clusters, average, centre shift, convergence test (labels unchanged -> strict; else
 * shift_tot <= tol).  Limits: D%4==0, D<=256, K<=32. */
#define DIC_KM_STATUS_WORDS 8
size_t dic_kmeans_workspace(int N, int D, int K, int n_runs);
int dic_kmeans_lloyd_iter(const float* X, const float* xnorm, int N, int D, int K, int n_runs,
                          float* centers, int32_t* labels, float* status,
                          void* workspace, size_t workspace_bytes, dic_stream_t stream);
/* The same iteration with the POINTS SHARDED over ranks (one process per GPU): each rank runs
 * dic_kmeans_lloyd_partial on its rows, the caller sums `stats` over ranks (one RCCL all-reduce of
 * n_runs * dic_kmeans_stats_words(D, K) doubles), and dic_kmeans_lloyd_finish completes the iteration identically on
 * every rank.  stats[run] = [ sums (K*D) | counts (K) | #labels changed (1) ], f64.  An empty cluster cannot be
 * relocated from partial data (the farthest point may live on another rank): finish then sets status[0] = 2 and leaves
 * the centres untouched; the caller re-runs that restart on unsharded data with dic_kmeans_lloyd_iter. */
size_t dic_kmeans_stats_words(int D, int K);
int dic_kmeans_lloyd_partial(const float* X, const float* xnorm, int N, int D, int K, int n_runs, const float* centers,
                             int32_t* labels, const float* status, double* stats, void* workspace, size_t workspace_bytes,
                             dic_stream_t stream);
int dic_kmeans_lloyd_finish(int D, int K, int n_runs, const double* stats, float* centers, float* status, dic_stream_t stream);
/* E-step only (KMeans.predict; also the final E-step after a tol stop):
 *   labels (n_runs,N) OVERWRITTEN; mindist (n_runs,N) or NULL = exact ||x-c_label||^2;
 *   inertia (n_runs) or NULL = sum of mindist (deterministic, f64 accumulation, f32 result). */
int dic_kmeans_predict(const float* X, int N, int D, int K, int n_runs, const float* centers,
                       int32_t* labels, float* mindist, float* inertia,
                       void* workspace, size_t workspace_bytes, dic_stream_t stream);
/* k-means++ helper (sklearn _kmeans.py:218-243 inner step), batched over restarts: L candidate rows
 * `cand` (int64 indices into X) in groups of `group` consecutive candidates per restart;
 * closest (L/group, N) = current closest squared distances of each restart (+inf for the first centre);
 * dist_out (L,N) = min(closest[l/group], ||x_i - X[cand_l]||^2), distances evaluated in f64 like
 * sklearn's float32 up-cast path; pot_out (L) f64 = sum_i dist_out[l,i]. */
size_t dic_kmeans_pp_workspace(int N, int L);
int dic_kmeans_pp_candidates(const float* X, int N, int D, const int64_t* cand, int L, int group,
                             const float* closest, float* dist_out, double* pot_out,
                             void* workspace, size_t workspace_bytes, dic_stream_t stream);
/* The same for the rows [row_lo, row_hi) only (points sharded over ranks): X, closest and dist_out keep their full
 * (., N) shapes, only those columns are read / written, pot_out = the partial potential of the range (the caller sums dist_out
 * and pot_out over ranks).  Candidate rows are still addressed in the full X. */
int dic_kmeans_pp_candidates_rows(const float* X, int N, int D, int row_lo, int row_hi, const int64_t* cand, int L, int group,
                                  const float* closest, float* dist_out, double* pot_out,
                                  void* workspace, size_t workspace_bytes, dic_stream_t stream);
/* out (n_rows, n) f64 = inclusive running sums along the rows of x (n_rows, n) f32, in f64: the stable_cumsum of scikit-learn's k-means++ sampling
 * (sklearn/cluster/_kmeans.py:218-243, as called from clustering_trainer.py:75-82 and p2_clustering_optK.py:260-389); deterministic summation order. */
int dic_cumsum_f64(const float* x, int n_rows, int n, double* out, dic_stream_t stream);

/* ------------------------------------------------------------------ bi-LSTM recurrence -----
 * Sequential half of one bidirectional torch.nn.LSTM layer with hidden size H = 128 (EncoderRNN /
 * DecoderRNN, clustering_interp.py:14-41; gate order i,f,g,o).  The caller (lstm.py) issues the
 * time-parallel GEMMs; bf16 tensors are passed as void*:
 *   gx    (R,B,2,4,H) bf16  X.W_ih^T + b_ih + b_hh per direction (0 = forward, 1 = reverse)
 *   whh   (2,4H,H)    bf16  recurrent weights;   whh_t (2,H,4H) bf16 their per-direction transposes
 *   h0,c0 (2,B,H) f32 or NULL;   out (R,B,2H) bf16;   hn,cn (2,B,H) f32
 *   gates (R,Bp,2,4,H) bf16 post-activation gates and cs (R,Bp,2,H) bf16 cell states (the forward carries c in f32), Bp = B rounded up to
 *   64: opaque, lane-native layout exchanged only between these two calls (both NULL for inference).
 * Backward: dout (R,B,2H) bf16 / dhn, dcn (2,B,H) f32 (each may be NULL) -> dgx (R,B,2,4,H) bf16
 * pre-activation gate gradients (the caller turns them into dX, dW_ih, dW_hh by GEMMs), dh0, dc0, and
 * dbias (2,4H) f32 or NULL = sum of dG over steps and batch rows (needs dic_lstm_bwd_workspace(B) bytes).
 * state_batch_major != 0: h0, c0, hn, cn and their gradients are laid out (B,2,H) instead of nn.LSTM's (2,B,H), so that
 * hn viewed as (B,2H) is the concatenated latent [h_fwd | h_rev] (clustering_interp.py:139) and feeds the decoder with no copy. */
int dic_lstm_fwd(const void* gx, int gx_lane_native, const void* whh, const float* h0, const float* c0, int R, int B, int H,
                 void* out, void* out_relu, float* hn, float* cn, void* gates, void* cs, int state_batch_major, int write_boundary,
                 dic_stream_t stream);
/* gx_lane_native == 2: the same with eight waves per workgroup (two per SIMD, 16 hidden units each; bit-identical results).
 * gx_lane_native != 0 (B a multiple of 64): gx is not row-major but in the opaque form dic_row_proj(..., lane_native_batch = B) writes --
 * the order of the recurrence kernel's MFMA accumulators, 1-KiB pieces per wave access -- and is read straight into registers a step
 * ahead (no LDS staging of the gx tile, one barrier per step). */
/* write_boundary != 0: `out` points at time slot 1 of an (R+2,B,2H) buffer (dic_lstm_dw's out_ext); the kernel also writes h0 (bf16;
 * zeros without one) into slot 0 [:, :H] and slot R+1 [:, H:], the recurrent inputs of the first forward / reverse step. */
/* out_relu (R,B,2H) bf16 or NULL: a second copy of the output with relu applied -- what DecoderRNN.forward reads of the encoder's
 * output (clustering_interp.py:38-41).  It leaves through the LDS tile of h the next step multiplies, as whole 256-B row halves;
 * the element-wise ReLU pass over (R,B,2H) disappears (its backward: dic_lstm_bwd's dout_of_relu). */
/* Same recurrence with the input projection computed in-kernel, for narrow inputs (the encoder's 3C channels):
 * G_t = x_t.wih^T + h_{t-1}.whh^T with x (R,B,I) bf16 and wih (2,4H,I) bf16, I == 32 (zero-pad narrower inputs; fold
 * the bias in as a constant-one input column whose weights are b_ih + b_hh).  Everything else as dic_lstm_fwd; the
 * backward is dic_lstm_bwd unchanged. */
int dic_lstm_fwd_proj(const void* x, const void* wih, const void* whh, const float* h0, const float* c0, int R, int B, int H,
                      int I, void* out, void* out_relu, float* hn, float* cn, void* gates, void* cs, int state_batch_major, int write_boundary,
                      int eight_waves, dic_stream_t stream);
/* eight_waves != 0: 512-thread workgroups, two waves per SIMD with 16 hidden units each (same results bit for bit): this variant's
 * per-step chain, not its bandwidth, bounds it, and the second wave on a SIMD fills the first one's gaps. */
size_t dic_lstm_bwd_workspace(int B);
int dic_lstm_bwd(const void* whh_t, const void* gates, const void* cs, const float* c0, const void* dout,
                 const float* dhn, const float* dcn, int R, int B, int H, void* dgx, float* dh0, float* dc0,
                 float* dbias, void* workspace, size_t workspace_bytes, int state_batch_major, int dout_of_relu, dic_stream_t stream);
/* dout_of_relu != 0: the consumer of `out` was relu(out) (the decoder rectifies the encoder output, clustering_interp.py:38-41) and
 * dout is the gradient of THAT: the kernel passes it where h_t > 0, read off the sign of tanh(c_t) it computes anyway (o_t is a
 * sigmoid) -- the element-wise ReLU backward pass over (R,B,2H) disappears. */

/* The same recurrence for the two regimes the 64-row bf16 kernels above do not serve (csrc/dic_lstm32.hip): dtype =
 * DIC_DTYPE_F32 -- every tensor f32, the recurrent product on v_mfma_f32_32x32x2_f32 (exact f32: the configuration of the 1e-5
 * parity tests, which round 1 left on MIOpen's nn.LSTM) -- and dtype = DIC_DTYPE_BF16 for small batches (the reference's own
 * B = 256: one 32-row tile per workgroup instead of two; round 4: one 16-row tile up to 2048 rows, v_mfma_f32_16x16x32_bf16, same results bit
 * for bit).  Element type T of gx, whh, out, gates, cs, dout, dgx follows dtype -- except that with DIC_DTYPE_F32X3 (round 6: eight waves per 32-row tile,
 * any batch size; gate non-linearities on the transcendental unit, ~3e-7 relative) dgx leaves as SPLIT PLANES: (2, R*B, 2*4H) bf16, plane 0 = bf16(dG),
 * plane 1 = bf16(dG - plane 0) -- the f32 tensor's bytes in the form dic_gemm_tn_planes / dic_gemm_nt_planes multiply without converting;
 * gates (R,Bp,2,4,H) and cs (R+1,Bp,2,H), Bp = B rounded up to 32, are an opaque lane-native layout exchanged between the two
 * calls of one (dtype, B) -- the 16- and 32-row kernels order it differently, and which pair runs is a function of B and the process environment
 * (DIC_REC_SIXTEEN, DIC_REC16_MAX) alone -- (time slot R of cs carries c0, so the backward takes no c0).  whh (2,4H,H); the backward takes either that (read transposed
 * once at start-up) or the transposed copy (2,H,4H) with whh_is_transposed != 0.
 * state_flags of the forward: bit 0 = the state tensors (h0, c0, hn, cn) are batch-major (B,2,H); bit 1 (round 3) = `out` is time slots
 * 1..R of an (R+2,B,2H) buffer and the kernel also writes h0 (zeros without one) into slot 0 [:, :H] / slot R+1 [:, H:] -- every step's
 * recurrent input for the weight-gradient kernels, as dic_lstm_fwd's `boundary` does (two fill / copy launches per LSTM less). */
#define DIC_DTYPE_F32 0
#define DIC_DTYPE_BF16 1
#define DIC_DTYPE_F32X3 2   /* dic_lstm_rec_fwd / _bwd only: f32 tensors, the recurrent products as three-term bf16 splits (hi.hi + lo.hi + hi.lo) on the bf16 matrix cores */
int dic_lstm_rec_fwd(int dtype, const void* gx, const void* whh, const float* h0, const float* c0, int R, int B, int H, void* out,
                     float* hn, float* cn, void* gates, void* cs, int state_flags, dic_stream_t stream);
/* dic_lstm_rec_fwd_proj (bf16, batches up to 4096): the same 32-row forward recurrence with the encoder's input projection inside the kernel -- x (R,B,I)
 * bf16 packed rows [3C features | 1 | 0...] as dic_sci_cci_fwd_packed writes them (I = 32 or 64), wih (2*4H, I) bf16 from dic_lstm_pack(bias_col = 1):
 * the (R,B,8H) gx tensor and the projection launch of nn.LSTM (clustering_interp.py:22) do not exist.  Other arguments as dic_lstm_rec_fwd. */
int dic_lstm_rec_fwd_proj(const void* x, const void* wih, const void* whh, const float* h0, const float* c0, int R, int B, int H, int I, void* out,
                          float* hn, float* cn, void* gates, void* cs, int state_flags, dic_stream_t stream);

/* dic_lstm_rec_fwd_proj_x3 (round 6): the x3 (DIC_DTYPE_F32X3) forward recurrence -- eight waves per 32-row tile, any batch size -- with the NARROW input
 * projection inside the kernel: x (R,B,ldx) f32 rows [features | 1 | 0...], wih (2*4H, ldx) f32 rows [W_ih | b_ih + b_hh | 0...] (dic_lstm_pack(DIC_DTYPE_F32,
 * bias_col = 1)), ldx a multiple of 4 up to 32; both are split into bf16 hi + lo on their way into LDS / registers and the product is hi.hi + lo.hi + hi.lo
 * like the recurrent one.  The f32 gx tensor of nn.LSTM's input projection (clustering_interp.py:22; 3.2 GB at 32 768 encounters) does not exist.  Other
 * arguments as dic_lstm_rec_fwd with f32 tensors. */
int dic_lstm_rec_fwd_proj_x3(const float* x, const float* wih, int ldx, const float* whh, const float* h0, const float* c0, int R, int B, int H, float* out,
                             float* hn, float* cn, float* gates, float* cs, int state_flags, dic_stream_t stream);

/* dic_lstm_fwd_xproj (bf16, H = 128, I = 256: the decoder; clustering_interp.py:30-41): the forward recurrence with the input projection x W_ih^T + b inside
 * the kernel -- gx (R,B,8H) is never formed.  x (R,B,256) bf16 raw rows (relu_x != 0: rectified on load, the F.relu between encoder and decoder), wih (2,4H,256),
 * whh (2,4H,H), bias (2,4H) bf16 as dic_lstm_pack writes them.  gates (R,Bp,2,4,H) / cs (R,Bp,2,H), Bp = B rounded up to 64, leave in the lane-native order
 * dic_lstm_bwd reads (c0 goes to the backward separately, as with dic_lstm_fwd).  out_r: optional (R,B,2H) relu(out), as dic_lstm_fwd's.  state_flags as
 * dic_lstm_rec_fwd. */
int dic_lstm_fwd_xproj(const void* x, const void* wih, const void* whh, const void* bias, const float* h0, const float* c0, int R, int B, int H, int I,
                       void* out, void* out_r, float* hn, float* cn, void* gates, void* cs, int state_flags, int relu_x, dic_stream_t stream);

size_t dic_lstm_rec_bwd_workspace(int B);
int dic_lstm_rec_bwd(int dtype, const void* whh, int whh_is_transposed, const void* gates, const void* cs, const void* dout,
                     const float* dhn, const float* dcn, int R, int B, int H, void* dgx, float* dh0, float* dc0, float* dbias,
                     void* workspace, size_t workspace_bytes, int state_batch_major, int dout_of_relu, dic_stream_t stream);

/* dic_lstm_dx_tile: the decoder LSTM's input gradient dX = dG . W_ih (the backward of nn.LSTM's input projection, clustering_interp.py:29-41; dg (N, 1024)
 * bf16 gate gradients of both directions as dic_lstm_bwd writes them) on 256 x 256 macro-tiles with nothing resident -- one persistent 8-wave workgroup per CU, dG slabs
 * (HBM) through a 3-slot and W_ih^T slabs (L2) through a 2-slot all-LDS-DMA ring, 16-B stores straight from the accumulators: every CU takes in its
 * row share of dG once.  w_ih_t (in_features = 256, gate_columns = 1024) bf16 = W_ih TRANSPOSED (k contiguous, like the rows of dg); dx (N, 256)
 * bf16 OVERWRITTEN.  N >= 256.  Replaces the last library GEMM of the bf16 step (nn.LSTM's backward: clustering_interp.py:29-41). */
int dic_lstm_dx_tile(const void* dg, const void* w_ih_t, int64_t N, int gate_columns, int in_features, void* dx, dic_stream_t stream);
/* dic_lstm_dx_tile_x3 (round 6): the same product for the f32 step on split products -- dX (N, 256) F32 = dG . W_ih with dG as the two bf16 planes
 * dic_lstm_rec_bwd(DIC_DTYPE_F32X3) writes (hi at dg_hi, lo dg_plane elements behind it, (N, 1024) each) and W_ih^T (256, 1024) split the same way by the
 * caller (hi at w_ih_t_hi, lo wt_plane elements behind it); every product hi.hi + lo.hi + hi.lo.  Same macro-tiles and LDS-DMA rings, a slab = both planes of
 * a 32-deep k range.  N >= 256.  Replaces dic_gemm_nt on the f32 operand (nn.LSTM's backward, clustering_interp.py:29-41). */
int dic_lstm_dx_tile_x3(const void* dg_hi, long dg_plane, const void* w_ih_t_hi, long wt_plane, int64_t N, int gate_columns, int in_features, float* dx,
                        dic_stream_t stream);

/* ------------------------------------------------------------------ bi-LSTM parameters --------
 * The eight f32 parameters of one bidirectional nn.LSTM layer (clustering_interp.py:22,35: weight_ih_l0, weight_hh_l0,
 * bias_ih_l0, bias_hh_l0, then the same four with the _reverse suffix) are passed as a HOST array of 8 device pointers in
 * that order.
 *   dic_lstm_pack: (dtype = DIC_DTYPE_BF16 or DIC_DTYPE_F32 selects the OUTPUT element type) -> wih (2*4H, Ip) bf16 [columns [0,I) = W_ih; column I = b_ih + b_hh when bias_col (dic_lstm_fwd_proj's
 *     constant-one input column); rest 0], whh (2,4H,H) bf16, whh_t (2,H,4H) bf16 or NULL, bias (2*4H) bf16 = b_ih + b_hh
 *     or NULL, wih_t (Ip, 2*4H) = wih transposed (dic_lstm_dx_tile's operand) or NULL.  One launch replaces the stack / add / cast / pad / transpose sequence of torch ops.
 *   dic_lstm_dw (encoder, packed input width Ip == 32): weight gradients from ONE pass over the gate gradients,
 *     dW_hh[d] = sum_t dG_t[d]^T h_prev_t[d] (h_{t-1} for d = 0, h_{t+1} for d = 1) and dW_ih[d] = sum_t dG_t[d]^T x_t[:, :I]
 *     (x (R,B,Ip) bf16).  out_ext (R+2,B,2H) bf16 = the layer's own output in time slots 1..R (pass &out_ext[1] to
 *     dic_lstm_fwd*), slot 0 [:, :H] = h0 of the forward direction and slot R+1 [:, H:] = h0 of the reverse direction (zeros
 *     without an h0): every step's recurrent input is then the row B above / below its dG row.  MFMA with transposed LDS
 *     reads.  With wih (2*4H, Ip) bf16 (dic_lstm_pack's) and dx_parts (2, R*B, Ip) bf16 given (both or neither), the same pass also
 *     writes the per-direction input gradients dx_parts[d] = dG[d] . W_ih[d] (columns [0, I), I <= 19; the caller adds the two
 *     directions) -- the third GEMM that used to re-read dG.  Deterministic two-stage reduction of the weight gradients, written
 *     (accumulate = 0) or added (accumulate = 1) straight into the
 *     parameter gradients `grads` (host array of 8 device pointers, same order; the bias entries are not touched).
 *   dic_lstm_dw_wide (decoder, input width I == 256 = the rectified encoder outputs, x (R,B,256) bf16): the same one-pass weight
 *     gradients -- four workgroups (direction x half of the gate rows) per chunk of rows, placed on one XCD so that the x / h tiles they
 *     share are served by its L2 -- instead of the three split-K library products that each re-read dG (decoder dW 0.90 -> see DESIGN.md).
 *   dic_lstm_unpack_grads: staging tensors dw_ih (2*4H, ldw) / dw_hh (2,4H,H) / dbias (2*4H) f32 (each may be NULL) ->
 *     the parameter gradients (dbias goes to bias_ih AND bias_hh). */
int dic_lstm_pack(int dtype, const float* const* params, int H, int I, int Ip, int bias_col, void* wih, void* whh, void* whh_t, void* bias,
                  void* wih_t, dic_stream_t stream);
size_t dic_lstm_dw_workspace(int R, int B);
int dic_lstm_dw(const void* dgx, const void* out_ext, const void* x, const void* wih, void* dx_parts, int R, int B, int H, int I, int Ip,
                float* const* grads, int accumulate, void* workspace, size_t workspace_bytes, dic_stream_t stream);
size_t dic_lstm_dw_wide_workspace(int R, int B);
int dic_lstm_dw_wide(const void* dgx, const void* out_ext, const void* x, int x_relu, int R, int B, int H, int I, float* const* grads, int accumulate,
                     void* workspace, size_t workspace_bytes, dic_stream_t stream);
/* dic_lstm_dw_x3 (round 6): the same weight gradients for the f32 step on split products (DIC_DTYPE_F32X3) -- dW_ih[d] = dG[d]^T . x, dW_hh[d] = dG[d]^T . h_prev[d],
 * every product hi.hi + lo.hi + hi.lo -- from ONE pass over the gate gradients in the form dic_lstm_rec_bwd(DIC_DTYPE_F32X3) writes them: two bf16 planes, hi at
 * dg_hi and lo dg_plane elements behind it, (R*B, 2*4H) each, streamed by LDS-DMA as they lie.  out_ext ((R+2)*B, 2H) f32 and x (R*B, ldx) f32 as the other f32
 * kernels take them (x_relu != 0: the LSTM ran on relu(x)).  I = 256 (the decoder; ldx = 256) or I <= ldx <= 32 with ldx a multiple of 4 (the encoder's rows
 * [features | 1 | 0...]; only columns [0, I) reach weight_ih).  R*B >= 16.  Narrow input, wih (2*4H, ldx) f32 (dic_lstm_pack) and dx_parts (4, R*B, ldx) f32 given:
 * four partial input gradients -- one per (direction, half of its gate rows) -- come out of the same pass (their sum is dX = dG . W_ih).  Replaces dic_gemm_tn / dic_gemm_nt on the f32 tensors (nn.LSTM's
 * backward, clustering_interp.py:14-41). */
size_t dic_lstm_dw_x3_workspace(int R, int B, int I);
int dic_lstm_dw_x3(const void* dg_hi, long dg_plane, const float* out_ext, const float* x, int ldx, int x_relu, const float* wih, float* dx_parts, int R, int B, int H,
                   int I, float* const* grads, int accumulate, void* workspace, size_t workspace_bytes, dic_stream_t stream);
int dic_lstm_unpack_grads(const float* dw_ih, int ldw, const float* dw_hh, const float* dbias, int H, int I, float* const* grads,
                          int accumulate, dic_stream_t stream);

/* ------------------------------------------------------------------ row-wise projection, 256 inputs ---
 * out (N,Nout) bf16 = x (N,256) . w (Nout,256)^T + bias (Nout) (bias bf16 or NULL), Nout a multiple of 256: the decoder LSTM's input
 * projection gx over all N = R*B rows (nn.LSTM inside DecoderRNN, clustering_interp.py:47-59) with the weights resident in
 * registers -- the library GEMM for this K = 256 shape cannot overlap its short main loop with its epilogue. */
int dic_row_proj(const void* x, const void* w, const void* bias, int64_t N, int in_features, int out_features, void* out, int lane_native_batch,
                 int relu_input, dic_stream_t stream);
/* relu_input != 0 (and x_relu of dic_lstm_dw_wide): x is the RAW output of the encoder LSTM and the product is taken of relu(x) -- the F.relu
 * between encoder and decoder (clustering_interp.py:38-41) applied to the operand on its way through the kernel, so that no rectified copy of
 * the encoder output exists in HBM. */
/* lane_native_batch = B > 0 (Nout = 1024 = 2 directions x 4 gates x 128 units, N = R*B, B a multiple of 64): out is written in the
 * lane-native form dic_lstm_fwd(gx_lane_native = 1) reads (same bytes, same values, another order); 0: row-major (N,Nout). */
/* The same for CompressFC's first layer Linear(256, 128) (rbf.py:111-125) in front of its training-mode BatchNorm1d: out (N,128) bf16 and
 * sums (2*128 + 1) f64 = [column sums of out | of out^2 | N] -- what dic_bn_colstats would compute in a second pass over out. */
size_t dic_row_proj_stats_workspace(int64_t N, int out_features);
int dic_row_proj_stats(const void* x, const void* w, const void* bias, int64_t N, int in_features, int out_features, void* out, double* sums,
                       void* workspace, size_t workspace_bytes, dic_stream_t stream);

/* ------------------------------------------------------------------ CompressFC first layer, backward ---
 * Linear(256, 128) over all N = B*R decoder rows (rbf.py:111-125, first layer; TimeDistributed utils.py:202-224): from ONE pass over
 * the rows, dx (N,256) bf16 = dz . W (or NULL) and dw (128,256) f32 = dz^T . x, for dz (N,128), x (N,256), w (128,256) bf16 -- instead of
 * two library GEMMs that each read dz.  MFMA with transposed LDS reads for the weight gradient; deterministic two-stage reduction. */
size_t dic_fc_bwd_workspace(int64_t N, int in_features, int out_features);
int dic_fc_bwd(const void* dz, const void* x, const void* w, int64_t N, int in_features, int out_features, void* dx, float* dw,
               void* workspace, size_t workspace_bytes, dic_stream_t stream);
/* The same with dz formed inside the kernel instead of read: the layer's own output z (N,128) bf16 goes through the backward of the
 * tail behind it -- BatchNorm1d(128, training) -> ReLU -> Dropout -> Linear(128, C) (rbf.py:114-124) -- on its way into LDS, with the
 * arithmetic of dic_bnhead_bwd_input (bit-identical dz): dv (N,C) f32 the gradient of the tail's output; mean, rstd, gamma, beta (128),
 * w2 (C,128) f32; sum_da, sum_dax (128) the column sums of dic_bnhead_bwd_reduce (summed over ranks); count (1) the global row count
 * of the batch moments (dic_bn_moments); relu / drop_p / rng as in dic_bnhead_bwd_input.  Compiled for C = 6. */
int dic_fc_bwd_bnhead(const void* z, const float* dv, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* w2,
                      const float* sum_da, const float* sum_dax, const float* count, int C, int relu, float drop_p, const uint64_t* rng,
                      const void* x, const void* w, int64_t N, int in_features, int out_features, void* dx, float* dw,
                      void* workspace, size_t workspace_bytes, dic_stream_t stream);

/* ------------------------------------------------------------------ CompressFC output layer ---
 * Linear(128, C) over all N = B*R decoder rows (rbf.py:111-125, last layer; TimeDistributed utils.py:202-224)
 * for small C (1..8, 12, 16): h (N,128) bf16, W (C,128) f32, b (C) f32 -> v (N,C) f32; backward:
 * dv (N,C) f32 -> dh (N,128) bf16, dW (C,128), db (C). */
int dic_head_fwd(const void* h, const float* W, const float* b, int64_t N, int K, int C, float* v, dic_stream_t stream);
size_t dic_head_bwd_workspace(int64_t N, int K, int C);
int dic_head_bwd(const void* h, const float* W, const float* dv, int64_t N, int K, int C, void* dh, float* dW, float* db,
                 void* workspace, size_t workspace_bytes, dic_stream_t stream);

/* ------------------------------------------------------------- CompressFC tail, fused ---------
 * BatchNorm1d(128) -> ReLU -> Linear(128, C) (rbf.py:116-123 with dropout p = 0 or eval mode) over N rows
 * without materialising the hidden activation.  z (N,128) bf16 = output of the first Linear; mean, rstd,
 * gamma, beta (128) f32; W (C,128), b (C) f32; C in 1..8.
 *   dic_bn_colstats:       sums[0:128] = sum_rows z, sums[128:256] = sum_rows z^2, sums[256] = N (f64, 257 entries; the caller
 *                          all-reduces the record first when the batch is sharded over ranks)
 *   dic_bn_moments:        that record -> mean, rstd = 1/sqrt(biased var + eps) (128 f32 each), count (1 f32), and -- when
 *                          running_mean / running_var are given -- nn.BatchNorm1d's running statistics (momentum < 0 =
 *                          cumulative average) and num_batches_tracked += 1, all in one launch
 *   dic_bnhead_fwd:        v (N,C) f32 = b + W relu(gamma (z - mean) rstd + beta)
 *   dic_bnhead_bwd_reduce: sums[(2+C)*128 + C] f32 = sum da | sum da*xhat | dW (C,128) | db (C), where
 *                          da = (dv W) 1[h > 0]; the first two rows are d beta and d gamma
 *   dic_bnhead_bwd_input:  dz (N,128) bf16 = gamma rstd (da - sum_da*inv_n - xhat sum_dax*inv_n); inv_n = 1 /
 *                          global row count in training mode (count != NULL: read from that device scalar instead); pass
 *                          zero sums for eval-mode BatchNorm.
 * relu = 0 drops the ReLU: BatchNorm1d(128) -> Linear(128, C), the tail of the auxiliary / fake-detection heads
 * (clustering_interp.py:43-87).  drop_p > 0 applies nn.Dropout(p) between the activation and the Linear (rbf.py:120): the
 * keep mask is a hash of (rng[0] = seed, rng[1] = call counter, element index) -- rng is a 2-word device buffer that the
 * caller keeps unchanged between a forward and its backward calls -- so no mask tensor exists. */
size_t dic_bn_colstats_workspace(int64_t N, int K);
int dic_bn_colstats(const void* z, int64_t N, int K, double* sums, void* workspace, size_t workspace_bytes, dic_stream_t stream);
int dic_bn_moments(const double* sums, int K, float eps, float momentum, float* running_mean, float* running_var,
                   int64_t* num_batches_tracked, float* mean, float* rstd, float* count, dic_stream_t stream);
int dic_bnhead_fwd(const void* z, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* W,
                   const float* b, int64_t N, int K, int C, int relu, float drop_p, const uint64_t* rng, float* v, dic_stream_t stream);
size_t dic_bnhead_bwd_workspace(int64_t N, int K, int C);
int dic_bnhead_bwd_reduce(const void* z, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* W,
                          const float* dv, int64_t N, int K, int C, int relu, float drop_p, const uint64_t* rng, float* sums,
                          void* workspace, size_t workspace_bytes, dic_stream_t stream);
int dic_bnhead_bwd_input(const void* z, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* W,
                         const float* dv, const float* sum_da, const float* sum_dax, double inv_n, const float* count, int64_t N, int K, int C, int relu,
                         float drop_p, const uint64_t* rng, void* dz, dic_stream_t stream);
/* The same four kernels on an f32 (N,128) pre-activation -- the f32 step ('x3' products: ops.mfma_linear writes z in f32): every value of the
 * BatchNorm -> ReLU -> Dropout -> Linear tail stays f32, no torch BatchNorm kernels, no library GEMM for the C-wide head. */
int dic_bn_colstats_f32(const float* z, int64_t N, int K, double* sums, void* workspace, size_t workspace_bytes, dic_stream_t stream);
int dic_bnhead_fwd_f32(const float* z, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* W,
                       const float* b, int64_t N, int K, int C, int relu, float drop_p, const uint64_t* rng, float* v, dic_stream_t stream);
int dic_bnhead_bwd_reduce_f32(const float* z, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* W,
                              const float* dv, int64_t N, int K, int C, int relu, float drop_p, const uint64_t* rng, float* sums,
                              void* workspace, size_t workspace_bytes, dic_stream_t stream);
int dic_bnhead_bwd_input_f32(const float* z, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* W,
                             const float* dv, const float* sum_da, const float* sum_dax, double inv_n, const float* count, int64_t N, int K, int C, int relu,
                             float drop_p, const uint64_t* rng, float* dz, dic_stream_t stream);


/* ------------------------------------------------- K-sweep statistics (p2, internal_eval) ------
 * One pass over all N^2 point pairs, nothing n x n materialised.  Replaces sklearn pairwise_distances per
 * cluster (p2_clustering_optK.py:334-351, gap-statistic inertia) and the distance work inside
 * silhouette_score / DunnIndex (internal_eval.py:37-126).
 * X (N,D) f32 with rows SORTED by cluster: cluster k = rows seg[k] .. seg[k+1]-1, seg (K+1) int32 on the
 * device, seg[0] = 0, seg[K] = N; D % 4 == 0; K <= 64.
 *   S (N,K) f32:     S[i][k] = sum over j in cluster k of ||x_i - x_j||   (f32 direct-difference distances)
 *   Dmin (N,K) f32:  Dmin[i][k] = min over j in cluster k of ||x_i - x_j|| (+inf for an empty cluster) [may be NULL]
 *   own_max (N):     farthest point of i's own cluster (0 for singletons)                              [may be NULL] */
int dic_cluster_pairdist(const float* X, const int32_t* seg, int N, int D, int K, float* S, float* Dmin, float* own_max,
                         dic_stream_t stream);

/* The same pass restricted to the pairs INSIDE a cluster -- all the gap statistic's inertia of a reference set needs (p2_clustering_optK.py:
 * 334-351: np.mean / np.sum of pairwise_distances(X[a == c]) per cluster): sum_c n_c^2 pairs instead of N^2.
 *   S_own (N) OVERWRITTEN: S_own[i] = sum over the points j of i's own cluster of ||x_i - x_j||  (rows sorted by cluster, as above). */
int dic_cluster_intra_sums(const float* X, const int32_t* seg, int N, int D, int K, float* S_own, dic_stream_t stream);
/* The per-cluster TOTALS of that pass on the matrix cores (round 6):  totals[c] (K) f64 OVERWRITTEN = sum over the ordered pairs (i, j) of cluster c of
 * ||x_i - x_j|| = np.sum(pairwise_distances(X[a == c])) (p2_clustering_optK.py:334-351) -- all the inertia of a gap-statistic reference set needs.  d^2 =
 * ||x_i||^2 + ||x_j||^2 - 2 x_i . x_j with x taken relative to centres[c] (K, D) f32 (any point near the cluster: its centroid) as ONE bf16 MFMA inner product of
 * augmented rows, every coordinate as hi + lo bf16 with the three leading partial products (the norms enter exactly): within 2e-7 of the f64 sum on the golden
 * clusterings.  X (N, D) f32 at row stride ldx, rows sorted by cluster as above, D <= 256, D % 4 == 0.  tiles (ntiles, 4) int32 on the device, sorted by
 * cluster: (first row of I, first row of J, end row of the cluster, cluster) for every pair of 256-row blocks I <= J of one cluster (block b of cluster c starts
 * at seg[c] + 256 b).  Only these pairs are visited (sum_c n_c^2 / 2 of the N^2).  Deterministic.  workspace: dic_cluster_intra_totals_workspace(N, K) bytes. */
/* The ROW SUMS of the all-pairs pass on the same machine (round 6):  S (N, K) f32 OVERWRITTEN, S[i][c] = sum over the points j of cluster c of ||x_i - x_j||
 * -- dic_cluster_pairdist's S without Dmin / own_max: what silhouette_score needs (internal_eval.py:112-123), 12 instead of 67 ms on 75 000 x 256.  Points
 * relative to ONE centre (1, D) f32 (their mean).  tiles (ntiles, 4) int32 on the device: (first row of a 256-row block I, first row of a 256-row block J of
 * cluster c, end row of c, output slot), sorted by (I, c, J); workgroup b of min(ntiles, 256) takes tiles [b per, (b + 1) per), per = ceil(ntiles / workgroups),
 * and a slot is a maximal run of one (I, c) inside one such range (slots numbered in list order).  group_start (blocks of I x K + 1) int32: the first slot of
 * every (I, c), in that order.  Deterministic.  workspace: dic_cluster_pair_rowsums_workspace(N, n_slots) bytes.  (Host side: cluster_stats._row_tile_list.) */
size_t dic_cluster_pair_rowsums_workspace(int64_t N, int n_slots);
int dic_cluster_pair_rowsums(const float* X, long ldx, const float* centre, int64_t N, int D, int K, const int32_t* tiles, int ntiles, const int32_t* group_start,
                             int n_slots, float* S, void* workspace, size_t workspace_bytes, dic_stream_t stream);
size_t dic_cluster_intra_totals_workspace(int64_t N, int K);
int dic_cluster_intra_totals(const float* X, long ldx, const int32_t* seg, const float* centres, int64_t N, int D, int K, const int32_t* tiles, int ntiles,
                             double* totals, void* workspace, size_t workspace_bytes, dic_stream_t stream);
/* out (K, D) f64 = per-cluster sums of the rows of values (N, D) f64 at row stride ldv, labels (N) int64 in [0, K) (others are skipped): the centroids of
 * scikit-learn's calinski_harabasz_score / davies_bouldin_score and the per-cluster distance sums of p2's gap statistic (internal_eval.py:112-147,
 * p2_clustering_optK.py:334-351).  Deterministic (no atomics, fixed order).  workspace: dic_segment_sum_workspace(D, K) bytes.  K <= 64. */
size_t dic_segment_sum_workspace(int D, int K);
int dic_segment_sum_f64(const double* values, long ldv, const int64_t* labels, int N, int D, int K, double* out, void* workspace, size_t workspace_bytes,
                        dic_stream_t stream);

/* ------------------------------------------------------------- optimisation step tail ---------
 * clip_grad_norm_ scaling + torch.optim.Adam(amsgrad=True, L2 weight decay) (pretrain_trainer.py:228-229, utils.py:83)
 * over one flat f32 bucket of n elements: p, g (scaled in place by *grad_scale, NULL = 1), exp_avg m, exp_avg_sq v,
 * max_exp_avg_sq vmax.  `step` = device pointer to the already incremented step count t (f32); `grad_scale` = device
 * pointer to the clip coefficient min(1, max_norm / (||g|| + 1e-6)); `active` = per-element byte mask or NULL (all):
 * elements with 0 are left untouched, as torch.optim skips parameters whose .grad is None.  `hyper` = device pointer to
 * [lr, beta1, beta2, eps, weight_decay] overriding the scalar arguments, or NULL: read on the device so that one captured hipGraph
 * of the step follows a learning-rate scheduler. */
int dic_adam_amsgrad_step(float* p, float* g, float* m, float* v, float* vmax, int64_t n, float lr, float beta1, float beta2,
                          float eps, float weight_decay, const float* step, const float* grad_scale, const unsigned char* active, const float* hyper,
                          dic_stream_t stream);
/* torch.nn.utils.clip_grad_norm_'s scalars for the flat gradient bucket (pretrain_trainer.py:228): out2[0] = ||g||_2,
 * out2[1] = min(1, max_norm / (||g||_2 + 1e-6)) -- the `grad_scale` of dic_adam_amsgrad_step.  Deterministic two-stage sum. */
size_t dic_grad_norm_workspace(int64_t n);
int dic_grad_norm_clip(const float* g, int64_t n, float max_norm, float* out2, void* workspace, size_t workspace_bytes, dic_stream_t stream);
/* dst[j][0..n[j]) += src[j][0..n[j]) for j < count (host arrays of device pointers / sizes) in one launch per 16 entries: the small
 * parameter gradients of the hot-path kernels added into their slots of the flat gradient bucket (what autograd's AccumulateGrad does
 * with one launch each between loss.backward() and the optimizer, pretrain_trainer.py:223-231). */
int dic_accumulate_many(const float* const* src, float* const* dst, const int* n, int count, dic_stream_t stream);

/* ---- row-streaming MFMA products (csrc/dic_gemm.hip) for the dense layers in the shapes no specialised kernel covers, and for the f32 step.
 * Replaces the library GEMMs behind nn.LSTM's input projections / nn.Linear (clustering_interp.py:14-41, rbf.py:111-125) and their
 * autograd gradients.  in_dtype DIC_DTYPE_BF16: one bf16 MFMA per product.  DIC_DTYPE_F32: operands split on the fly into bf16 hi + lo
 * pieces and multiplied as hi.hi + lo.hi + hi.lo in f32 accumulators ("bf16x3": products good to ~2^-17, at 5x the exact-f32 MFMA rate).
 *   dic_gemm_nt:  Y[m][n] = sum_k act(A[m][k]) W[n][k] (+ bias[n]);  A (M,K) rows at stride lda, W (N,K) rows at stride ldw (both of
 *                 in_dtype), Y (M,N) of out_dtype at stride ldy; relu_a != 0: act = max(., 0).  K, lda, ldw multiples of 4 (f32) / 8 (bf16)
 *                 elements, operands 16-B aligned.  An input gradient dX = dY.W is the same call with W handed over transposed.
 *   dic_gemm_tn:  D[n][k] (+)= sum_m A[m][n] X[m][k] for k < kcols;  A (M,N) at stride lda, X (M,K) at stride ldx (both in_dtype), D f32
 *                 (N,kcols) at stride ldd; the M rows are cut into chunks whose f32 partial products go through `workspace`
 *                 (dic_gemm_tn_workspace bytes) and are summed in a fixed order in f64: deterministic.  accumulate != 0: added to D. */
int dic_gemm_nt(int in_dtype, int out_dtype, const void* A, long lda, const void* W, long ldw, const float* bias, long M, int N, int K,
                void* Y, long ldy, int relu_a, dic_stream_t stream);
/* dic_x3_row_proj: out (N, out_features) f32 = act(x (N,256) f32) . w (out_features,256)^T + bias, every product a three-term bf16 split, for the
 * 256-input projections of the x3 f32 step (the decoder LSTM's input projection, out_features = 1024; CompressFC's Linear(256,128)): weights split once and
 * resident in registers, x tiles streamed through LDS (csrc/dic_gemm.hip).  out_features: 128 or a multiple of 256; relu_input != 0: act = max(., 0). */
int dic_x3_row_proj(const float* x, const float* w, const float* bias, int64_t N, int in_features, int out_features, float* out, int relu_input,
                    dic_stream_t stream);
size_t dic_gemm_tn_workspace(long M, int N, int K, int K2);
/* X2 (M,K2) at stride ldx2 (or NULL, K2 = 0): a second right-hand operand multiplied in the SAME pass over A, D2 (N,K2) f32 at stride ldd2 (+)= A^T.X2
 * -- dW_ih = dG^T.x and dW_hh = dG^T.h_prev read the gate gradients once.  relu_x != 0: the first product runs on max(X, 0). */
int dic_gemm_tn(int in_dtype, const void* A, long lda, const void* X, long ldx, long M, int N, int K, float* D, long ldd, int kcols,
                const void* X2, long ldx2, int K2, float* D2, long ldd2, int accumulate, int relu_x, void* workspace, size_t workspace_bytes, dic_stream_t stream);
/* Split-plane A operands (round 6).  The x3 recurrence backward (dic_lstm_rec_bwd, DIC_DTYPE_F32X3) writes the gate gradients -- f32 in nn.LSTM's backward,
 * clustering_interp.py:14-41 -- as TWO bf16 planes, hi = bf16(x) at A_hi and lo = bf16(x - hi) a_plane elements behind it (x = hi + lo to 2^-17, the same
 * bytes as f32); these take them as they lie -- no conversion of A in the loop -- against f32 W / X (split on the way in) and produce what dic_gemm_nt /
 * dic_gemm_tn produce for the f32 tensor hi + lo.  lda in bf16 elements; K (nt) / N (tn) and lda multiples of 8. */
int dic_gemm_nt_planes(const void* A_hi, long a_plane, long lda, const float* W, long ldw, const float* bias, long M, int N, int K, float* Y, long ldy,
                       dic_stream_t stream);
int dic_gemm_tn_planes(const void* A_hi, long a_plane, long lda, const float* X, long ldx, long M, int N, int K, float* D, long ldd, int kcols,
                       const float* X2, long ldx2, int K2, float* D2, long ldd2, int accumulate, int relu_x, void* workspace, size_t workspace_bytes, dic_stream_t stream);

/* DBSCAN without the distance matrix (csrc/dic_dbscan.hip): p2_clustering_optK.py:82-85,90-168 and p4_clustering_final.py:181-236 build
 * pairwise_distances(X) and fit DBSCAN(eps, min_samples, metric='precomputed') on it; these recompute the distances tile by tile on the matrix cores.
 * X (N, D) f32 at row stride ldx, D <= 256, D % 4 == 0 (zero-pad narrower points), N < 2^30, 16-B aligned.  Neighbour rule (sklearn's): (i, j) are
 * neighbours for eps e iff f32(||x_i - x_j||^2) <= thresholds[e], thresholds[e] the largest f32 s with sqrt_f32(s) <= eps under NumPy's promotion of the
 * caller's eps (dbscan.py); the self pair counts.  Thresholds lie in [0, 2^100) (eps < 2^50); one beyond returns DIC_ERR_UNSUPPORTED.  One workspace (dic_dbscan_workspace(N, D) bytes) serves the counting pass and, unchanged, every
 * components pass after it (it holds the split planes of the points).
 *   dic_dbscan_counts: counts (n_eps, N) int32 OVERWRITTEN = |N_eps(i)| for every eps (n_eps <= 16) in ONE pair pass; centre (1, D) f32 = the mean of the
 *       points.  A pair whose approximate d^2 lies within the derived error bound of some threshold is a BAND pair: appended to band (capacity, 4) int32 as
 *       (i, j, neighbour mask, 0) and decided exactly (f64 difference form) by a second kernel.  *n_band (host) = the number of band pairs found; more than
 *       `capacity` returns DIC_ERR_WORKSPACE (counts incomplete; run again with capacity >= *n_band).  Reads *n_band back: synchronises `stream`.
 *   dic_dbscan_components_pass: one label pass of eps eps_index (threshold = thresholds[eps_index]) over the core graph, core = counts_e[i] >= min_samples
 *       (counts_e = row eps_index of counts; band / n_band as dic_dbscan_counts left them).  labels (N) int32, initialised by the caller to 0..N-1: every
 *       core point takes the smallest label of its core neighbours and hooks its root to it (atomicMin), then labels jump to their roots.  *changed (device
 *       int32, zeroed by the caller) is set to 1 when a label moved.  border (N) int32 OVERWRITTEN: for a non-core point, the smallest label among its core
 *       neighbours (0x7f7f7f7f: none).  Repeat until a pass leaves *changed at 0; then labels[i] (core i) = the smallest core index of i's component and
 *       border holds, per border point, the root of its smallest-numbered neighbouring cluster (sklearn's _dbscan_inner).  Deterministic results. */
size_t dic_dbscan_workspace(int64_t N, int D);
int dic_dbscan_counts(const float* X, long ldx, const float* centre, int64_t N, int D, const float* thresholds, int n_eps, int32_t* counts, int32_t* band,
                      int64_t capacity, int64_t* n_band, void* workspace, size_t workspace_bytes, dic_stream_t stream);
int dic_dbscan_components_pass(int64_t N, int D, float threshold, int eps_index, const int32_t* counts_e, int min_samples, const int32_t* band, int64_t n_band,
                               int32_t* labels, int32_t* border, int32_t* changed, void* workspace, size_t workspace_bytes, dic_stream_t stream);

/* k-th neighbour distances without the distance matrix (csrc/dic_knn.hip): p2_clustering_optK.py:110-112 takes
 * NearestNeighbors(n_neighbors=k).fit(X).kneighbors(X)[0][:, -1] for its k-distance graph; the same quantity is OPTICS' core distance (dic_optics_order below takes it).
 * X, ldx, centre, N, D as for dic_dbscan_counts (D <= 256, D % 4 == 0, N < 2^30, 16-B aligned; centre (1, D) f32 = the mean of the points); 1 <= k <= N.
 *   dic_knn_kth_distance: kth (N) f64 OVERWRITTEN = the k-th smallest of { |x_i - x_j| : j = 0..N-1 }, the self pair included (k = 1 gives 0): the f64 square
 *       root of the f64 difference-form squared distance of the f32 coordinates, the value at the exact rank.  The split-bf16 tile products only narrow the
 *       search (4 counting pair passes with per-row thresholds); the pairs they cannot rank -- the candidates -- are listed by one more pair pass, group of
 *       rows by group of rows, and ranked exactly.  candidate_budget = the bytes of list storage inside the workspace (12 per candidate; <= 0: the default,
 *       384 MiB; never more than 12 N^2), which sizes the groups and nothing else: the result does not depend on it.  stats (HOST, 5 int64, may be NULL):
 *       counting passes, groups, the longest list, the candidates of all rows, the candidate_budget the longest list needs.  A row whose list alone exceeds
 *       the budget returns DIC_ERR_WORKSPACE with stats filled (run again with candidate_budget >= stats[4]).  Reads list sizes back: synchronises `stream`.
 *       Deterministic results. */
size_t dic_knn_workspace(int64_t N, int D, int64_t candidate_budget);
int dic_knn_kth_distance(const float* X, long ldx, const float* centre, int64_t N, int D, int64_t k, double* kth, int64_t candidate_budget, int64_t* stats,
                         void* workspace, size_t workspace_bytes, dic_stream_t stream);

/* Exact k-nearest-neighbour lists without the distance matrix (csrc/dic_knn.hip): NearestNeighbors(n_neighbors=k, algorithm='brute').fit(X).kneighbors(Q), the
 * lists knn.py's kneighbors, NearestNeighbors and knn_transfer_labels (p4's --transfer knn) are built on.  X (N, D) f32, row stride ldx: the index points;
 * Q (M, D) f32, row stride ldq: the queries, or NULL for the self join (every index point queries; M and ldq ignored).  centre (1, D) f32 = the mean of
 * the index points (any point near the data: it conditions the approximate products and never reaches the result).  D <= 256, D % 4 == 0, ldx % 4 == 0,
 * ldq % 4 == 0, 1 <= k <= min(N, 1024), N + M < 2^30, X, Q, centre and the workspace 16-B aligned -- the rules of dic_knn_kth_distance.
 *   dic_knn_neighbors: dist (M or N, k) f64 and idx (M or N, k) int32, DEVICE, OVERWRITTEN.  Row q holds the k index points j with the smallest keys
 *       (d^2(q, j), j) in lexicographic order, sorted ascending by that key: d^2 = the f64 difference-form squared distance of the f32 coordinates (the
 *       quantity dic_knn_kth_distance ranks, csrc/dic_exactd2.h), dist = its f64 square root, ties in distance broken by the smaller index.  The self pair of
 *       a self join is an ordinary pair with d^2 = 0; a query is never a neighbour.  dist[:, k - 1] of the self join is dic_knn_kth_distance's result bit
 *       for bit.  Nothing M x N is stored: four counting pair passes over the query row blocks x index column blocks bracket every row's k-th distance, one
 *       more pair pass lists every index point the bracket cannot exclude (k plus a few on ordinary data, up to N with duplicates), and one workgroup per
 *       row computes the exact d^2 of its list, radix-selects the key of rank k, and sorts the k survivors in LDS.  candidate_budget, stats and the
 *       DIC_ERR_WORKSPACE protocol are dic_knn_kth_distance's (12 bytes per list entry; the result does not depend on the budget).  Reads list sizes back:
 *       synchronises `stream`.  Two calls give the same bits. */
size_t dic_knn_neighbors_workspace(int64_t N, int64_t M, int D, int64_t candidate_budget);
int dic_knn_neighbors(const float* X, long ldx, int64_t N, const float* Q, long ldq, int64_t M, const float* centre, int D, int k, double* dist, int32_t* idx,
                      int64_t candidate_budget, int64_t* stats, void* workspace, size_t workspace_bytes, dic_stream_t stream);

/* Neighbour RANKS without the distance matrix (csrc/dic_knn_rank.hip): where does j stand among the neighbours of i -- the counterpart of dic_knn_neighbors,
 * which returns the neighbour at a given rank.  knn.py's neighbor_ranks and embedding_quality.py (trustworthiness, continuity) are built on it.
 * THE DEFINITION, stated here once.  Points are f32; d2(i, l) = the f64 difference-form squared distance of csrc/dic_exactd2.h.  The order of row i is the
 * order of dic_knn_neighbors: by the key (d2(i, l), l), ties in distance settled by the smaller index.
 *   rank(i, j) = 1 + #{ l != i : (d2(i, l), l) < (d2(i, j), j) }   for j != i:
 *       the 1-based position of j in row i of the self join's idx at k = N after the row's own index i is dropped (the rule t-SNE's lists follow; with
 *       duplicates i need not come first in its own list, and a duplicate of i is a neighbour like any other).
 *   A target j == i or j outside [0, N) (absent: write -1) has rank 0.
 * What embedding_quality.py makes of it (Venna and Kaski 2001), X the points and Y their map, kNN_Z(i) = the k nearest OTHER points of i in space Z:
 *   trustworthiness  T(k) = 1 - 2 / (N k (2N - 3k - 1)) * sum_i sum_{j in U_i} (rank_X(i, j) - k),  U_i = kNN_Y(i) \ kNN_X(i);  k < N / 2.
 *   continuity       C(k): the same with the two spaces swapped -- kNN_X(i) \ kNN_Y(i), ranked on the map.
 *   neighbours kept  mean_i |kNN_X(i) n kNN_Y(i)| / k.
 *   MAP PRECISION: the map is f64 and this machinery f32; map-side lists and ranks are those of the map ROUNDED TO f32 (at |Y| around 50 a 4e-6 grid).
 * Self join only.  X, ldx, centre, N, D as for dic_knn_neighbors (D <= 256, D % 4 == 0, ldx % 4 == 0, N < 2^30, 16-B aligned; centre (1, D) f32 = the mean
 * of the points).  targets (N, m) int32 and ranks (N, m) int32, DEVICE, ranks OVERWRITTEN; 1 <= m <= 1023 (more, or D > 256: DIC_ERR_UNSUPPORTED).
 *   dic_knn_ranks: one kernel computes the exact d2 of every target; ceil(m / 8) counting pair passes (8 targets = 16 per-row thresholds each) count the
 *       pairs the approximate products place certainly before each target; the pairs inside a target's band -- the ones they cannot place -- are listed by
 *       as many pair passes, group of rows by group of rows, and decided by (d2, index) in f64.  The approximate d2 never decides a rank.
 *       candidate_budget = the bytes of list storage inside the workspace (8 per band pair and target; <= 0: the default, 384 MiB), which sizes the groups
 *       and nothing else: the result does not depend on it.  stats (HOST, 5 int64, may be NULL): counting passes, groups, the longest row's band pairs, the
 *       band pairs of all rows, the candidate_budget the longest row needs.  A row whose bands alone exceed the budget returns DIC_ERR_WORKSPACE with stats
 *       filled (run again with candidate_budget >= stats[4]).  Reads list sizes back: synchronises `stream`.  Two calls give the same bits. */
size_t dic_knn_ranks_workspace(int64_t N, int D, int m, int64_t candidate_budget);
int dic_knn_ranks(const float* X, long ldx, const float* centre, int64_t N, int D, const int32_t* targets, int m, int32_t* ranks, int64_t candidate_budget,
                  int64_t* stats, void* workspace, size_t workspace_bytes, dic_stream_t stream);

/* A TEST INSTRUMENT (csrc/dic_pairtile_probe.hip), not an operator: the approximate squared distances a_ij of the shared pair-tile loop (csrc/dic_pairtile.h),
 * which dic_dbscan_*, dic_knn_*, dic_meanshift_members and dic_kmedoids_delta_pass decide on in registers and never store, written out so that
 * tests/test_gpu_pairtile.py can hold them to the header's bound |a_ij - d^2_ij| < 2^-12 (n_i + nmax_J).  Nothing in the package calls it.
 * X, ldx, centre, N, D as for dic_knn_kth_distance (D <= 256, D % 4 == 0, ldx % 4 == 0, 16-B aligned), N <= 65536; nblk = ceil(N / 256).  The planes are
 * prepared as the consumers prepare them (pad_norm >= 0, a power of two or 0: the norm the 256 padding points present as operand j), then ONE pair pass
 * walks tiles tile0 .. tile0 + ntiles - 1 of the row-major list of the nblk^2 256 x 256 tiles (ntiles = 0: all from tile0 on) on `grid` workgroups (0: the
 * consumers' own choice, min(ntiles, 256)).  All DEVICE: out (nblk 256, nblk 256) f32, out[i][j] = a_ij for every (i, j) of a walked tile, padding rows and
 * columns included, other entries untouched (the caller fills it with NaN beforehand); visits (nblk, nblk) int32, += 1 per walk of tile (I, J) (the caller
 * zeroes it); nrm (N + 256) f32 and bmax (nblk) f32 OVERWRITTEN = the norms and per-block largest norms the loop's consumers read (0 for padding rows). */
size_t dic_pairtile_probe_workspace(int64_t N, int D);
int dic_pairtile_probe(const float* X, long ldx, const float* centre, int64_t N, int D, float pad_norm, int64_t tile0, int64_t ntiles, int grid, float* out,
                       int32_t* visits, float* nrm, float* bmax, void* workspace, size_t workspace_bytes, dic_stream_t stream);

/* Shared-nearest-neighbour clustering on the neighbour lists (csrc/dic_snn.hip; Jarvis & Patrick 1973; Ertoz, Steinbach & Kumar 2003); no upstream counterpart.
 * THE DEFINITION, which snn.py, p2, p4 and the tests hold to.  k = n_neighbors, 2 <= k <= min(N, 1024).  L(i) = row i of the self join's idx (N, k) int32 from
 * dic_knn_neighbors: the k index points with the smallest (d^2, index) keys, the point itself an ordinary neighbour (L(i) contains i unless k or more exact
 * duplicates with smaller indices precede it; nothing below relies on it).
 *   similarity  for column c, j = L(i)[c]:  sim[i, c] = |L(i) n L(j)|  if j != i and i is in L(j) (a MUTUAL pair), else 0.  Symmetric: sim of (i, j) read
 *               from row i equals sim of (j, i) read from row j.
 *   density     density[i] = #{c : sim[i, c] >= eps}, eps an integer, 1 <= eps <= k.
 *   core        i is a core point iff density[i] >= min_samples, min_samples >= 0.  min_samples = 0 makes every point core: Jarvis-Patrick clustering, the
 *               components of the mutual graph thresholded at eps, an isolated point a cluster of its own.
 *   clusters    the connected components of the core points under the edges sim >= eps between two cores; cluster id = the rank of the component's smallest
 *               core index (dbscan.py's numbering).
 *   border      a non-core point with at least one edge sim >= eps to a core point takes the cluster of the core j with the largest sim; on equal sim the
 *               smaller j.
 *   noise       everything else: -1.
 * All results are integers; two calls give the same values.  idx, sim, density, labels, border, changed: DEVICE, 4-B aligned.  N < 2^30.
 *   dic_snn_similarity: sim (N, k) int32 OVERWRITTEN, every entry.  An entry of idx outside [0, N) is treated as absent from its list and is never used as a
 *       row index (its sim is 0): garbage lists give garbage counts, never an out-of-range access.  One pass over the lists, N k^2 entries read.
 *   dic_snn_components_pass: one label pass over the sparse graph, then a pointer-jump launch -- the protocol of dic_dbscan_components_pass.  density (N)
 *       int32 as defined above (torch: (sim >= eps).sum(1)).  labels (N) int32, initialised by the caller to 0..N-1: every core point takes the smallest label
 *       among itself and its strong core neighbours and hooks its root to it (atomicMin), then labels jump to their roots.  *changed (int32, zeroed by the
 *       caller) is set to 1 when a label moved.  Repeat until a pass leaves *changed at 0; then labels[i] (core i) = the smallest core index of i's
 *       component.  border (N) int32 OVERWRITTEN by every pass with the same values: for a border point the core j it belongs to under the rule above (its
 *       cluster is that of labels[border[i]]), -1 for core and noise points. */
int dic_snn_similarity(const int32_t* idx, int64_t N, int k, int32_t* sim, dic_stream_t stream);
int dic_snn_components_pass(const int32_t* idx, const int32_t* sim, int64_t N, int k, int eps, const int32_t* density, int min_samples, int32_t* labels,
                            int32_t* border, int32_t* changed, dic_stream_t stream);

/* OPTICS' ordering without the distance matrix (csrc/dic_optics.hip): p2_clustering_optK.py:86-88,171-223 fits sklearn.cluster.OPTICS; this is its main loop
 * in the self-consistent form sklearn has with metric='precomputed' on the f64 difference-form distances d of the f32 points.  X, ldx, N, D as for
 * dic_knn_kth_distance (D <= 256, D % 4 == 0, N < 2^30, X and the workspace 16-B aligned).  core (N) f64, DEVICE, in: the core distances, already set to inf
 * above max_eps and rounded as np.around(., 15) rounds (around15(v) = rint(v * 1e15) / 1e15) -- dic_knn_kth_distance(k = min_samples) supplies the values,
 * and its distances are bit for bit this file's (csrc/dic_exactd2.h), which the tie-breaking by index relies on.  max_eps >= 0, inf allowed.
 *   dic_optics_order: ordering (N) int32, reachability (N) f64, predecessor (N) int32, all OVERWRITTEN.  reachability = inf, predecessor = -1, nothing
 *       processed; N times: p = the unprocessed point of smallest reachability (ties, inf included: the smallest index) is appended to ordering; if core[p]
 *       is finite, every unprocessed q with d(p, q) <= max_eps takes r = around15(max(d(p, q), core[p])) and predecessor p where r < reachability[q].
 *       One launch per step, a row pass over X that also finds the next p (the workgroup arriving last reduces the others' minima); the N - 1 launches are
 *       enqueued on `stream` without synchronising and the call returns while they run: the results are complete when the stream has drained.  No launch
 *       waits for another workgroup.  The workspace (dic_optics_workspace(N, D) bytes, O(N)) holds the processed flags, the workgroup minima, the current
 *       point and the arrival counter.  Deterministic results. */
size_t dic_optics_workspace(int64_t N, int D);
int dic_optics_order(const float* X, long ldx, int64_t N, int D, const double* core, double max_eps, int32_t* ordering, double* reachability,
                     int32_t* predecessor, void* workspace, size_t workspace_bytes, dic_stream_t stream);

/* HDBSCAN's minimum spanning tree without the distance matrix (csrc/dic_hdbscan.hip): Prim's walk over the mutual-reachability graph
 * mr(p, q) = max(core[p], core[q], d(p, q)) as sklearn.cluster.HDBSCAN(metric='precomputed', algorithm='brute') takes it on the f64 difference-form
 * distances d of the f32 points (_linkage.pyx: mst_from_mutual_reachability).  X, ldx, N, D as for dic_optics_order (D <= 256, D % 4 == 0, N < 2^30, X and
 * the workspace 16-B aligned).  core (N) f64, DEVICE, in: the distances to the min_samples-th neighbour, the point itself counted, UNROUNDED --
 * dic_knn_kth_distance(k = min_samples) supplies the values, and its distances are bit for bit this file's (csrc/dic_exactd2.h): every edge into a sparse
 * point weighs exactly that point's core distance, and the tie-breaking by index relies on equal bits.
 *   dic_hdbscan_mst: ordering (N) int32, reachability (N) f64, predecessor (N) int32, all OVERWRITTEN.  reachability = inf, predecessor = -1, point 0 is first;
 *       N - 1 times: the current point p is in the tree; every q outside it with mr(p, q) < reachability[q] (strictly) takes that value and predecessor p; the
 *       point outside the tree of smallest reachability (ties: the smallest index) is appended to ordering and becomes p.  reachability[q] is the weight at
 *       which q joined (inf for point 0) and predecessor[q] its neighbour in the tree (-1 for point 0); sklearn's edge record of step i is
 *       (ordering[i], ordering[i + 1], reachability[ordering[i + 1]]).  One launch per step, as dic_optics_order: the N - 1 launches are enqueued on `stream`
 *       without synchronising (N = 1: none), the results are complete when the stream has drained, and no launch waits for another workgroup.  The
 *       workspace (dic_hdbscan_workspace(N, D) bytes, O(N)) holds the in-tree flags, the workgroup minima, the current point and the arrival counter.
 *       Deterministic results. */
size_t dic_hdbscan_workspace(int64_t N, int D);
int dic_hdbscan_mst(const float* X, long ldx, int64_t N, int D, const double* core, int32_t* ordering, double* reachability, int32_t* predecessor,
                    void* workspace, size_t workspace_bytes, dic_stream_t stream);

/* Consensus clustering from a label matrix and the average-linkage agglomeration of its consensus distance (csrc/dic_consensus.hip): the p2 / p4
 * `--cluster_method consensus` branches (p4_clustering_final.py:241-287 reads labels "generated outside": Monti-style consensus clustering with a k-means
 * base clusterer, ConsensusClusterPlus' conventions).  L (N, ldl) uint8, DEVICE, 16-B aligned: L[i, h] for h < H is the label 0..K-1 (K <= 254) of point i in
 * resample h, or 0xFF where resample h left the point out; ldl % 16 == 0 and the columns H..ldl-1 hold 0xFF.  2 <= N < 2^30, 1 <= H <= 65535.  For a pair, in
 * integers: both = #{h: L_ih != FF and L_jh != FF}, agree = #{h: L_ih == L_jh != FF}; consensus M(i, j) = agree / both, 0 when both == 0.
 *   dic_consensus_pairs: one tiled pass over the pairs for each of the outputs asked for (NULL: skipped; at least one):
 *       hist (DIC_CONSENSUS_BINS + 1) u64 OVERWRITTEN: over the unordered pairs i < j, the exact count of t = ceil(B agree / both) in integer arithmetic,
 *           (B agree + both - 1) / both, t = 0 when both == 0 (B = DIC_CONSENSUS_BINS).
 *       D (N, N) f64 OVERWRITTEN: 1.0 - (double)agree / (double)both, one f64 division and one subtraction; 1.0 when both == 0; 0 on the diagonal; (i, j) and
 *           (j, i) are stored from one register: exactly symmetric.
 *       rowsum (N, K) f64 OVERWRITTEN = sum over j != i with y[j] == c of M(i, j), each term (double)agree / (double)both, summed in f64 in a fixed order (the
 *           rows are sorted by cluster first and every row has one owner; no floating-point atomics): needs y (N) int32, DEVICE, 1 <= K <= 254 and the
 *           workspace (dic_consensus_pairs_workspace(N, H, K) bytes; K = 0: no rowsum, no workspace needed).  A y[j] outside 0..K-1 belongs to no cluster.
 *       Every output has the same bits whichever others are asked for, and from call to call.  Enqueued on `stream` without synchronising.
 *   dic_linkage_average: scipy.cluster.hierarchy.linkage(., 'average') on the SQUARE symmetric matrix D (N, N) f64, DEVICE, which is DESTROYED: the
 *       nearest-neighbour chain with scipy's tie-breaking -- size[i] = 1, chain empty; N - 1 times: an empty chain becomes [smallest live i]; repeat x =
 *       chain[-1], y = the live i != x of smallest (D[x, i], i) except that chain[-2] wins a tie with that minimum, until y == chain[-2], else append y; pop
 *       both, (x, y) = (min, max), record, size[x] = 0, size[y] = nx + ny, D[i, y] = D[y, i] = (nx D[i, x] + ny D[i, y]) / (nx + ny) for every live i != y, each
 *       operation correctly rounded in f64 and none contracted.  records (N - 1, 4) f64 OVERWRITTEN: (x, y, height, nx + ny) per merge in the order the
 *       merges happen: NOT sorted by height and not relabelled (consensus.average_linkage does both on the host).  One launch of one workgroup per repeat of
 *       the inner loop, 3 (N - 1) launches in all, enqueued without synchronising; size, chain and the counters live in the workspace
 *       (dic_linkage_average_workspace(N) bytes, O(N); its last 256 B begin with three int32: chain length, merges done, launches that pushed or merged);
 *       no workgroup waits for another.  8 N^2 bytes of D: the caller checks that they fit.  Deterministic. */
#define DIC_CONSENSUS_BINS 100
size_t dic_consensus_pairs_workspace(int64_t N, int H, int K);
int dic_consensus_pairs(const unsigned char* L, long ldl, int64_t N, int H, const int32_t* y, int K, unsigned long long* hist, double* rowsum, double* D,
                        void* workspace, size_t workspace_bytes, dic_stream_t stream);
size_t dic_linkage_average_workspace(int64_t N);
int dic_linkage_average(double* D, int64_t N, double* records, void* workspace, size_t workspace_bytes, dic_stream_t stream);

/* Ward's agglomerative clustering without the distance matrix (csrc/dic_ward.hip): scipy.cluster.hierarchy.linkage(X, 'ward') on the f32 points X (N, ldx),
 * DEVICE, 16-B aligned, D % 4 == 0 <= 256, ldx % 4 == 0, 2 <= N < 2^30; X is only read.  A live cluster i has a size n_i, the f64 coordinate sums S_i and the
 * centroid C_i = S_i / n_i (one rounded division per coordinate when the cluster is made); d2(i, j) = (2 n_i n_j / (n_i + n_j)) * sum_k (C_i[k] - C_j[k])^2, the
 * sum in f64 in dic_exactd2.h's order, the factor in f64 and symmetric in i and j, nothing contracted; the height of a merge is sqrt(d2).  A merge of a < b
 * leaves S_b = S_a + S_b, n_b = n_a + n_b, C_b = S_b / n_b, n_a = 0.
 *   dic_ward_linkage: the nearest-neighbour chain with scipy's tie-breaking, as dic_linkage_average states it (an empty chain starts at the smallest live
 *       index; the neighbour is the lexicographic minimum of (d2, index); chain[-2] wins a tie).  records (N - 1, 4) f64 OVERWRITTEN: (a, b, height,
 *       n_a + n_b) per merge in the order the merges happen: NOT sorted by height and not relabelled (ward.ward_linkage does both on the host).  One launch per
 *       repeat of the chain's inner loop -- a row pass over the live centroids by at most 256 workgroups, whose minimum the last workgroup to arrive takes in
 *       the same launch, as dic_optics_order -- 3 (N - 1) launches in all, enqueued on `stream` without synchronising; no workgroup waits for another.  The
 *       workspace (dic_ward_workspace(N, D) bytes, linear in N: S and C, 2 x 8 N D bytes, the sizes, the chain, the workgroup minima and the state) ends
 *       with 256 B that begin with four int32: chain length, merges done, launches that pushed or merged, smallest live index.  Deterministic. */
size_t dic_ward_workspace(int64_t N, int D);
int dic_ward_linkage(const float* X, long ldx, int64_t N, int D, double* records, void* workspace, size_t workspace_bytes, dic_stream_t stream);

/* Gaussian mixtures with diagonal (cov_type 0) or spherical (cov_type 1) covariances by EM, every operation in f64 (csrc/dic_gmm.hip; sklearn.mixture.
 * GaussianMixture's model).  X (N, ldx) f32, DEVICE, 16-B aligned, only read; D % 4 == 0 <= 256, ldx % 4 == 0, 2 <= N < 2^30, 1 <= K <= DIC_MAX_CLUSTERS,
 * n_runs >= 1; D0 (1 <= D0 <= D) is the true feature count, the columns D0 .. D - 1 are zero padding and add nothing, their variances are skipped.  All
 * parameters are f64 on the DEVICE, per restart: weights (n_runs, K), means (n_runs, K, D), variances (n_runs, K, D) (spherical: one value repeated over D);
 * shift (D) is shared.  Every x enters as x' = (double)x - shift, and `means` holds mu' = mu - shift.
 *   E-step: M_ik = sum_d (x'_id - mu'_kd)^2 / v_kd;  log p_ik = log w_k - (D0 log 2 pi + M_ik) / 2 - (sum_{d < D0} log v_kd) / 2;  lse_i = logsumexp_k log p_ik
 *       with the maximum subtracted;  log r_ik = log p_ik - lse_i;  the lower bound is mean_i lse_i.
 *   M-step: n_k = sum_i r_ik + 10 * 2^-52;  mu'_k = sum_i r_ik x'_i / n_k;  v_kd = sum_i r_ik x'_id^2 / n_k - mu'_kd^2 + reg_covar (spherical: the mean over
 *       d < D0);  w_k = (n_k / N) / sum_k (n_k / N).
 * Sums over rows are per-workgroup f64 partials in the workspace (dic_gmm_workspace bytes, 16-B aligned), added in block order by a second kernel: no
 * floating-point atomics, two calls give the same bits, and a restart's bits do not depend on the restarts beside it.  Nothing synchronises `stream`.
 *   dic_gmm_em_iter: one E+M pass for every restart whose done flag is clear; done restarts keep their parameters.  status (n_runs, DIC_GMM_STATUS_WORDS) f64
 *       IN/OUT: [0] done, [1] iterations run, [2] 1 if stopped by the tolerance, [3] the last lower bound (set -inf before the first iteration), [4] tol (IN),
 *       [5] max_iter (IN), [6] internal, [7] unused; zero [0..2] before the first iteration.  The pass appends its lower bound to
 *       lower_bounds[run * lb_stride + iterations] (dropped beyond lb_stride), and sets done when |lb_t - lb_(t-1)| < tol or iterations reaches max_iter; the
 *       M-step of the converging iteration is kept, as in sklearn.
 *   dic_gmm_estep: the E-step of ONE parameter set.  Outputs, each optional (NULL): lse (N) f64, log_resp (N, K) f64, labels (N) int32 (the first maximum of
 *       log p), sum_lse (1) f64 (sum_i lse_i in fixed order).
 *   dic_gmm_mstep_labels: the M-step from hard labels (labels (n_runs, N) int32: one-hot responsibilities; a label outside 0 .. K - 1 gives a row of zeros) or
 *       from responsibilities (resp (n_runs, N, K) f64) -- exactly one of the two -- through the accumulation of the EM pass. */
#define DIC_GMM_STATUS_WORDS 8
size_t dic_gmm_workspace(int64_t N, int D, int K, int n_runs);
int dic_gmm_em_iter(const float* X, long ldx, int64_t N, int D, int D0, int K, int n_runs, int cov_type, double reg_covar, const double* shift, double* weights,
                    double* means, double* variances, double* status, double* lower_bounds, int lb_stride, void* workspace, size_t workspace_bytes,
                    dic_stream_t stream);
int dic_gmm_estep(const float* X, long ldx, int64_t N, int D, int D0, int K, const double* shift, const double* weights, const double* means,
                  const double* variances, double* lse, double* log_resp, int32_t* labels, double* sum_lse, void* workspace, size_t workspace_bytes,
                  dic_stream_t stream);
int dic_gmm_mstep_labels(const float* X, long ldx, int64_t N, int D, int D0, int K, int n_runs, int cov_type, double reg_covar, const double* shift,
                         const int32_t* labels, const double* resp, double* weights, double* means, double* variances, void* workspace,
                         size_t workspace_bytes, dic_stream_t stream);

/* Variational Bayesian Gaussian mixtures with diagonal (cov_type 0) or spherical (cov_type 1) covariances, every operation in f64 (csrc/dic_bgmm.hip, bgmm.py;
 * sklearn.mixture.BayesianGaussianMixture's model, stated at the head of csrc/dic_bgmm.hip).  X, ldx, N, D, D0, K, n_runs, shift and the workspace rules as for
 * dic_gmm_*: x' = (double)x - shift, `means` (n_runs, K, D) holds the shifted m_k, `variances` (n_runs, K, D) the normalised v_kd (spherical: one value
 * repeated over d < D0); in the padding m = 0 and v = 1.  prior_type 0 is the Dirichlet process (stick breaking), 1 the Dirichlet distribution.  Priors:
 * gamma0 > 0 (weight concentration), kappa0 > 0 (mean precision), nu0 > D0 - 1 (degrees of freedom), mean_prior (D) f64 DEVICE, shifted (m0 - shift, 0 in the
 * padding), cov_prior (D) f64 DEVICE (spherical: one value repeated).  comp (n_runs, DIC_BGMM_COMP_WORDS, K) f64 DEVICE holds per component, row by row:
 * 0 n_k, 1 kappa_k, 2 nu_k, 3 l_k = -(sum_{d < D0} log v_kd) / 2 - (D0 log nu_k) / 2, 4 log_lambda_k, 5 sum_{j < D0} lgamma((nu_k - j) / 2), 6 a_k (process)
 * or alpha_k (distribution), 7 b_k (process; 0 otherwise), 8 E[log pi_k], 9 lc_k, the constant of log p_ik = lc_k - M_ik / 2.
 * Sums over rows are per-workgroup f64 partials (dic_bgmm_workspace bytes), added in block order; every other sum is sequential in index order: no
 * floating-point atomics, two calls give the same bits, and a restart's bits do not depend on the restarts beside it.  Nothing synchronises `stream`.
 *   dic_bgmm_init: the M-step from hard labels (n_runs, N) int32 (a label outside 0 .. K - 1 gives a row of zeros) or from responsibilities (n_runs, N, K)
 *       f64 -- exactly one of the two -- and the first constants: writes means, variances and every row of comp.
 *   dic_bgmm_em_iter: one E+M pass, the reduction and the finish step for every restart whose done flag is clear.  status and lower_bounds as
 *       dic_gmm_em_iter, but the lower bound is the variational bound, a sum over the rows and not a mean.
 *   dic_bgmm_estep: the E-step of ONE parameter set: log_const (K) is row 9 of its comp.  Outputs as dic_gmm_estep, each optional.
 *   dic_bgmm_special_probe: digamma_out[i] = psi(x[i]) by the kernels' own device function (NaN for x <= 0) and lgamma_out[i] = lgamma(x[i]) by the device
 *       library, for n values on the DEVICE, on the null stream; either output may be NULL.  For the tests. */
#define DIC_BGMM_COMP_WORDS 10
size_t dic_bgmm_workspace(int64_t N, int D, int K, int n_runs);
int dic_bgmm_init(const float* X, long ldx, int64_t N, int D, int D0, int K, int n_runs, int cov_type, int prior_type, double reg_covar, double gamma0,
                  double kappa0, double nu0, const double* shift, const double* mean_prior, const double* cov_prior, const int32_t* labels, const double* resp,
                  double* means, double* variances, double* comp, void* workspace, size_t workspace_bytes, dic_stream_t stream);
int dic_bgmm_em_iter(const float* X, long ldx, int64_t N, int D, int D0, int K, int n_runs, int cov_type, int prior_type, double reg_covar, double gamma0,
                     double kappa0, double nu0, const double* shift, const double* mean_prior, const double* cov_prior, double* means, double* variances,
                     double* comp, double* status, double* lower_bounds, int lb_stride, void* workspace, size_t workspace_bytes, dic_stream_t stream);
int dic_bgmm_estep(const float* X, long ldx, int64_t N, int D, int D0, int K, const double* shift, const double* log_const, const double* means,
                   const double* variances, double* lse, double* log_resp, int32_t* labels, double* sum_lse, void* workspace, size_t workspace_bytes,
                   dic_stream_t stream);
int dic_bgmm_special_probe(const double* x, int64_t n, double* digamma_out, double* lgamma_out);

/* Fuzzy c-means (Bezdek) with the fuzzifier m, every operation in f64 (csrc/dic_fcm.hip, fcm.py).  X, ldx, N, D, K, n_runs, shift and the workspace rules as
 * for dic_gmm_* (there is no D0: the padding columns are zero in the points and in the centres and add nothing); m must be finite and > 1.  centers
 * (n_runs, K, D) f64 DEVICE holds v' = v - shift; every x enters as x' = (double)x - shift.  With p = 1 / (m - 1):
 *   d2_ik = sum_d (x'_id - v'_kd)^2;  dmin_i = min_k d2_ik;
 *   dmin_i > 0:  r_ik = dmin_i / d2_ik,  t_ik = r_ik if m == 2 exactly, else exp(p log r_ik),  u_ik = t_ik / sum_k t_ik;
 *   dmin_i == 0: u_ik = [d2_ik == 0] / #{k : d2_ik == 0};
 *   w_ik = u_ik^2 if m == 2, else exp(m log u_ik), 0 where u_ik == 0;  v'_k = sum_i w_ik x'_i / sum_i w_ik (a component without weight keeps its centre);
 *   J = sum_ik w_ik d2_ik,  S2 = sum_ik u_ik^2,  SE = sum_ik u_ik log u_ik (0 log 0 = 0), all from the centres that ENTERED the pass.
 * Sums over rows are per-workgroup f64 partials (dic_fcm_workspace bytes: K + K D + 3 doubles per workgroup and restart), added in block order: no
 * floating-point atomics, two calls give the same bits, and a restart's bits do not depend on the restarts beside it.  Nothing synchronises `stream`.
 *   dic_fcm_workspace: bytes of the workspace (16-B aligned) of the other calls, 0 for arguments outside the limits.
 *   dic_fcm_iter: one iteration of every restart whose done flag is clear; centers are updated in place, done restarts keep theirs.  status (n_runs,
 *       DIC_GMM_STATUS_WORDS) f64 IN/OUT, the words as for dic_gmm_em_iter with [3] the last J.  The pass writes J_t to objectives[run * obj_stride +
 *       iterations] (dropped beyond obj_stride) and sets done after iteration t >= 2 if |J_(t-1) - J_t| <= tol J_(t-1) ([2] = 1), or when iterations
 *       reaches max_iter; the first iteration never stops, and the update of the stopping iteration is kept.
 *   dic_fcm_memberships: ONE centre set.  Outputs, each optional (NULL): u (N, K) f64, labels (N) int32 (the first maximum of u), d2 (N, K) f64,
 *       sums (3) f64 = J, S2, SE in block order. */
size_t dic_fcm_workspace(int64_t N, int D, int K, int n_runs);
int dic_fcm_iter(const float* X, long ldx, int64_t N, int D, int K, int n_runs, double m, const double* shift, double* centers, double* status,
                 double* objectives, int obj_stride, void* workspace, size_t workspace_bytes, dic_stream_t stream);
int dic_fcm_memberships(const float* X, long ldx, int64_t N, int D, int K, double m, const double* shift, const double* centers, double* u, int32_t* labels,
                        double* d2, double* sums, void* workspace, size_t workspace_bytes, dic_stream_t stream);

/* Gaussian mixtures with full (cov_type 2) or tied (cov_type 3) covariances by EM, every operation in f64, the products on the f64 matrix cores
 * (csrc/dic_gmm_full.hip, gmm_full.py; sklearn.mixture.GaussianMixture's model).  X, D, D0, ldx, N, K, n_runs, shift, weights (n_runs, K) and means
 * (n_runs, K, D) as for dic_gmm_*: x' = (double)x - shift, `means` holds mu' = mu - shift, the columns D0 .. D - 1 are zero padding.  Kc = K for full and 1 for
 * tied covariances.  Per restart, f64 on the DEVICE: covariances (n_runs, Kc, D, D), symmetric; prec_chol (n_runs, Kc, D, D), upper triangular (exactly 0 below
 * the diagonal); log_det (n_runs, Kc).  In the padding (an index >= D0) C and P are the identity: the padding adds exactly 0 to M and to log_det.
 *   E-step: y_ik = (x'_i - mu'_k) P_k;  M_ik = sum_d y_ikd^2;  log p_ik = log w_k - (D0 log 2 pi + M_ik) / 2 + log_det_k,  log_det_k = sum_{d < D0} log P_k,dd;
 *       lse_i = max_k log p_ik + log sum_k exp(log p_ik - max) (k in order), log r_ik = log p_ik - lse_i; the lower bound is mean_i lse_i.
 *   M-step: n_k = sum_i r_ik + 10 * 2^-52;  mu'_k = sum_i r_ik x'_i / n_k;  w_k = (n_k / N) / sum_k (n_k / N).
 *       full: C_k = S_k / n_k - mu'_k mu'_k^T + reg_covar I,  S_k = sum_i r_ik x'_i x'_i^T.
 *       tied: C = (T - sum_k n_k mu'_k mu'_k^T) / sum_k n_k + reg_covar I,  T = sum_i x'_i x'_i^T (scatter_total (D, D): it does not depend on r, is formed once
 *       per fit -- dic_gmm_full_mstep with compute_total != 0 writes it -- and only read afterwards).
 *       Both are sklearn 1.7.2's _estimate_gaussian_covariances_full / _tied in shifted coordinates and expanded form.
 *   Factor: C = L L^T, P = L^-T, by columns in this order:  for j = 0 .. D0 - 1:  s_i = C_ij, then s_i = s_i - L_it L_jt for t = 0 .. j - 1 ascending (one rounded
 *       product, one rounded difference), for every i >= j;  L_jj = sqrt(s_j);  L_ij = s_i / L_jj.  Then for every column j of P, c = j .. 0 descending:
 *       P_jj = 1 / L_jj;  P_cj = -(sum_{t = c + 1 .. j} L_tc P_tj) / L_cc, the sum from 0.0 with t ascending.  log_det = sum_d log P_dd, d ascending from 0.0.
 *       A pivot s_j that is not a finite positive number sets the restart's status word [7] to 1 and its done flag [0]; that matrix's P becomes the identity
 *       and its log_det 0, so nothing downstream reads a NaN, and the other restarts go on.
 * Sums over rows: the E-step's per-workgroup partials (sum lse, sum_i r_ik, sum_i r_ik x'_i; at most 256 workgroups per restart, their rows a function of N
 * alone) are added in block order; S_k / T are computed on and below the block diagonal of 16 x 16 tiles per row slab -- slabs(N, m) = max(1, min(ceil(N / 256),
 * ceil(128 / m))) for m matrices per restart (m = K for S_k, 1 for T): a function of N and K alone -- and the slab matrices are added in slab order by the kernel
 * that also mirrors the lower triangle, so C == C^T bit for bit.  No floating-point atomics; two calls give the same bits; a restart's bits do not depend on
 * the restarts beside it; nothing synchronises `stream`.
 *   dic_gmm_full_workspace: bytes of the workspace (16-B aligned) of the other calls, 0 for arguments outside the limits.  With a256(w) = 8 w rounded up to 256,
 *       B = min(256, ceil(N / 64)) workgroups and R = n_runs:  a256(R N K) [log r] + a256(R B (K (D + 1) + 1)) [partials] + a256(R K) [n_k]
 *       + a256(R K slabs(N, K) D^2) (full) or a256(slabs(N, 1) D^2) (tied) [slab matrices] + a256(R Kc D^2) [L^T of the factor].
 *   dic_gmm_full_em_iter: one E+M pass, factor included, for every restart whose done flag is clear.  status and lower_bounds as dic_gmm_em_iter, and
 *       status[7] = 1 after an ill-defined covariance.
 *   dic_gmm_full_estep: the E-step of ONE parameter set; the optional outputs of dic_gmm_estep.
 *   dic_gmm_full_mstep: the M-step, factor included, from hard labels (n_runs, N) int32 or responsibilities (n_runs, N, K) f64 -- exactly one.  status
 *       (n_runs, DIC_GMM_STATUS_WORDS): only [0] and [7] are written, after an ill-defined covariance.
 *   dic_gmm_full_factor: covariances (n_runs, n_mats, D, D) -> prec_chol, log_det, status[0] / [7]; its workspace is 8 n_runs n_mats D^2 bytes. */
size_t dic_gmm_full_workspace(int64_t N, int D, int K, int n_runs, int cov_type);
int dic_gmm_full_em_iter(const float* X, long ldx, int64_t N, int D, int D0, int K, int n_runs, int cov_type, double reg_covar, const double* shift,
                         double* weights, double* means, double* covariances, double* prec_chol, double* log_det, const double* scatter_total, double* status,
                         double* lower_bounds, int lb_stride, void* workspace, size_t workspace_bytes, dic_stream_t stream);
int dic_gmm_full_estep(const float* X, long ldx, int64_t N, int D, int D0, int K, int cov_type, const double* shift, const double* weights, const double* means,
                       const double* prec_chol, const double* log_det, double* lse, double* log_resp, int32_t* labels, double* sum_lse, void* workspace,
                       size_t workspace_bytes, dic_stream_t stream);
int dic_gmm_full_mstep(const float* X, long ldx, int64_t N, int D, int D0, int K, int n_runs, int cov_type, double reg_covar, const double* shift,
                       const int32_t* labels, const double* resp, double* scatter_total, int compute_total, double* weights, double* means, double* covariances,
                       double* prec_chol, double* log_det, double* status, void* workspace, size_t workspace_bytes, dic_stream_t stream);
int dic_gmm_full_factor(const double* covariances, int n_runs, int n_mats, int D, int D0, double* prec_chol, double* log_det, double* status, void* workspace,
                        size_t workspace_bytes, dic_stream_t stream);

/* Spectral clustering on the symmetrised k-neighbour graph (csrc/dic_spectral.hip, spectral.py): sklearn 1.7.2's
 * SpectralClustering(affinity='nearest_neighbors'), stated here once.
 *   L(i): the list of the k nearest neighbours of point i from dic_knn_neighbors, self join (the point itself its first entry), 2 <= k.  A: the 0/1 matrix of
 *   the lists.  W = 0.5 (A + A^T), entries 0.5 or 1, its diagonal dropped before the degrees are taken (scipy's laplacian).  deg_i = sum_j W_ij > 0 (k >= 2:
 *   every point has an off-diagonal neighbour), dd_i = sqrt(deg_i).  M = D^-1/2 W D^-1/2 has its spectrum in [-1, 1]; sklearn's Laplacian is I - M.  Wanted:
 *   the m largest eigenpairs (theta_1 >= .. >= theta_m, V) of M.  Embedding = V / dd row-wise, then every eigenvector's entry of largest magnitude made
 *   positive, the first one on equal magnitude (_deterministic_vector_sign_flip).  Labels: k-means (n_init = 10) or sklearn's cluster_qr on the first K
 *   columns of the embedding.  The multiplicity of the eigenvalue 1 is the number of connected components of the graph.
 * The graph is a CSR without its diagonal: indptr (N + 1) int64, indices (nnz) int32 ascending within a row, weight (nnz) one byte per entry, 1 = 0.5 and
 * 2 = 1.0 (the kernel takes 0.5 * weight), dd (N) f64; all on the DEVICE and only read.  M is never stored: M_ij = (0.5 weight) / (dd_i * dd_j), one
 * multiplication and one division in f64 -- symmetric in i and j bit for bit.  Rows may be of any length up to N (hub points).  An entry of indices outside
 * [0, N) is absent from its row, and indptr is clamped to [0, nnz]: nothing outside the arrays is read.
 * Blocks are (N, b) f64 row-major on the DEVICE, 1 <= b <= 64, 1 <= N < 2^30, 8-B aligned.  Every kernel is f64 throughout, has no floating-point atomics and
 * no workgroup that waits for another; every result has the same bits from call to call, and the order of every sum is a function of the operands' shapes
 * (N, b, the row's entries) alone, not of the device or the grid.  Nothing synchronises `stream`.
 *   dic_spectral_spmm: Y = alpha (M X) + beta X + gamma Z, the fused step of a three-term recurrence (Z NULL: no third term).  Y must not be X; Y may be Z.
 *       (M X)[i, c]: with g = the power of two >= b and e = 64 / g, the entries of row i at positions s, s + e, s + 2 e, .. are added in ascending order, each
 *       by one fma into the running sum, for every s < e; the e sums are then added in the xor tree s ^ 1, s ^ 2, ...
 *   dic_spectral_gram: G (b, b) row-major OVERWRITTEN = A^T B.  Every workgroup sums 128 consecutive rows in ascending order (fma); the partials
 *       (dic_spectral_gram_workspace(N, b) bytes, 8-B aligned) are added in block order by a second kernel.
 *   dic_spectral_rotate: Y = X C, C (b, b) row-major on the DEVICE, the sum over p ascending (fma).  Y must not be X. */
int dic_spectral_spmm(const int64_t* indptr, const int32_t* indices, const unsigned char* weight, const double* dd, int64_t N, int64_t nnz, int b,
                      const double* X, const double* Z, double alpha, double beta, double gamma, double* Y, dic_stream_t stream);
size_t dic_spectral_gram_workspace(int64_t N, int b);
int dic_spectral_gram(const double* A, const double* B, int64_t N, int b, double* G, void* workspace, size_t workspace_bytes, dic_stream_t stream);
int dic_spectral_rotate(const double* X, const double* C, int64_t N, int b, double* Y, dic_stream_t stream);

/* Mean shift with the flat kernel (csrc/dic_meanshift.hip, meanshift.py): sklearn 1.7.2's cluster/_mean_shift.py written as f64 arithmetic, stated here once.
 *   Inputs: X (N, D) f32 points; x'_j = (double)x_j - c, c (D) f64 the column means.  A seed s is f64.  Bandwidth h > 0, t = h * h in f64.
 *   Members: m(s) = { j : d2(s, j) <= t }.  d2 is the f64 difference form in the lane order of csrc/dic_exactd2.h: lane l holds coordinates 4 l .. 4 l + 3,
 *       an fma chain over its four terms (s_k - (double)x_jk)^2 in coordinate order, then wave_sum's xor tree; the seed coordinate is f64 and the point
 *       coordinate is promoted exactly.  The comparison is <=: a point at exactly h is a member.
 *   One shift: |m(s)| = 0: the seed is finished with count 0 (and dropped later).  Otherwise s_new = c + (sum_{j in m(s)} x'_j) / |m(s)|,
 *       moved = ||s_new - s||_2, s = s_new; the seed is finished if moved <= 1e-3 h or if it has already completed max_iter iterations, otherwise its
 *       iteration count goes up by one (sklearn's loop order: max_iter = 0 is exactly one shift).  The count kept for a seed is |m| of its last shift.  The
 *       new position depends on the old one only through the member set: with equal member sets rounding does not accumulate over the iterations.
 *   Centres: the finished seeds with count > 0, sorted descending by (count, tuple(coordinates)) (sklearn's sorted(.., reverse=True)), walked in that order:
 *       a centre not yet suppressed suppresses every other centre within d2 <= t of it and survives.  The survivors in walk order are cluster_centers_.
 *   Labels: labels_[j] = the nearest centre by d2 (the centre as the f64 operand), ties to the smaller centre index; with cluster_all = False, -1 where
 *       d2 > t.  predict is the same rule without orphans.
 *   Seeds: every point by default, an explicit array, or sklearn's get_bin_seeds.  estimate_bandwidth(X, quantile) = the f64 mean of the k-th neighbour
 *       distance (dic_knn_kth_distance, the point itself included), k = max(1, int(N quantile)).
 * X (N, ldx) f32, DEVICE, 16-B aligned, only read; D % 4 == 0 <= 256 (zero-padded columns add nothing), ldx % 4 == 0.  Seeds and centres are packed (rows, D)
 * f64 on the DEVICE; `centre` (D) f32 is the centre of the bf16 planes ((float)c), `shift` (D) f64 is c.  0 < bandwidth < 2^50.
 *   dic_meanshift_prepare: the planes of the points in a workspace of dic_meanshift_workspace(N, M_max) bytes (16-B aligned), once per fit; M_max = the most
 *       seeds one members pass will take (N + M_max + 256 < 2^30).
 *   dic_meanshift_members: mask (M, ceil(N / 32)) uint32, DEVICE, OVERWRITTEN: bit j & 31 of word j >> 5 of row s is set iff j in m(seed s); bits >= N are
 *       0.  1 <= M <= M_max.  A pass over (seed, point) tiles on the matrix cores decides every pair whose approximate d2 lies clear of t and lists the rest
 *       (BAND pairs: band (capacity, 4) int32, DEVICE, 16-B aligned), which a second kernel decides with the exact d2.  More band pairs than `capacity`
 *       returns DIC_ERR_WORKSPACE with *n_band (HOST) the number needed (mask incomplete; run again with capacity >= *n_band).  Reads *n_band back:
 *       synchronises `stream`.  The mask is a fixed function of the inputs.
 *   dic_meanshift_shift: one shift of every seed s < M whose done[s] is 0 (others are left as they are), from its mask row: counts[s] = |m|, and by the rule
 *       above seeds[s] (IN/OUT), iters[s] (IN/OUT) and done[s] (IN/OUT; zero both before the first shift).  sums (M, D) f64, optional (NULL): the member sums
 *       sum_j x'_j of the seeds shifted by this call.  A 0/1 by f64 product on the f64 matrix cores, the points in ascending order; no floating-point
 *       atomics, two calls give the same bits.  Nothing synchronises `stream`.
 *   dic_meanshift_nearest: for n_rows rows -- X f32 (stride ldx) or R f64 (packed), exactly one non-NULL -- against C >= 1 centres: idx (n_rows) int32 the
 *       nearest centre, ties to the smaller index, and d2 (n_rows) f64 its exact d2 (each optional, not both NULL).  Nothing synchronises `stream`. */
size_t dic_meanshift_workspace(int64_t N, int64_t M_max);
int dic_meanshift_prepare(const float* X, long ldx, int64_t N, int D, const float* centre, int64_t M_max, void* workspace, size_t workspace_bytes,
                          dic_stream_t stream);
int dic_meanshift_members(const float* X, long ldx, int64_t N, int D, const float* centre, const double* seeds, int64_t M, int64_t M_max, double bandwidth,
                          uint32_t* mask, int32_t* band, int64_t capacity, int64_t* n_band, void* workspace, size_t workspace_bytes, dic_stream_t stream);
int dic_meanshift_shift(const float* X, long ldx, int64_t N, int D, const double* shift, const uint32_t* mask, int64_t M, double* seeds, double bandwidth,
                        int max_iter, int32_t* counts, int32_t* iters, int32_t* done, double* sums, dic_stream_t stream);
int dic_meanshift_nearest(const float* X, long ldx, const double* R, int64_t n_rows, int D, const double* centres, int C, int32_t* idx, double* d2,
                          dic_stream_t stream);

/* k-medoids (PAM) with the Euclidean distance (csrc/dic_kmedoids.hip, kmedoids.py), stated here once.  All arithmetic is f64.
 *   Distances: d(o, c) = sqrt(exact_d2(x_o, x_c)), exact_d2 as csrc/dic_exactd2.h defines it (the f64 difference form of the f32 rows in its lane order).
 *   For medoids m_0 .. m_{K-1} (distinct rows of X): n(o) = the slot of the nearest medoid, ties to the smaller slot; dn(o) the distance to it, ds(o) the
 *       distance to the second nearest (+inf at K = 1); TD = sum_o dn(o).
 *   BUILD: the first medoid is the c that minimises sum_o d(o, c); each further one is the non-medoid c that minimises
 *       g(c) = sum_o [min(d(o, c), dn(o)) - dn(o)]; ties to the smaller index.  The BUILD medoids of K are the first K of those of any larger K.
 *   SWAP: steepest descent (the original PAM's result, with FastPAM1's shared removal term).  Per iteration, for every non-medoid c and every slot i:
 *       Delta(c, i) = sum_o [min(d(o, c), dn(o)) - dn(o)] + sum_{o: n(o) = i} [min(d(o, c), ds(o)) - min(d(o, c), dn(o))].
 *       Take the smallest Delta, ties to the smaller c, then the smaller i.  If it is not < 0: stop, converged.  Otherwise c goes into slot i and the next
 *       iteration starts, up to max_iter iterations.
 *   Order of the sums over o (two runs give the same bits): TD: a workgroup of 1024 threads, thread t adds dn[t], dn[t + 1024], .. ascending, then a binary
 *       tree over the 1024 partials (stride 512, 256, .., 1).  g and Delta: 16 waves, wave w adds its terms for o = w, w + 16, .. ascending -- g and, per slot,
 *       r_i = the second sum -- then g = the waves' g in wave order, r_i likewise, Delta(c, i) = g + r_i.
 * X (N, ldx) f32, DEVICE, 16-B aligned, only read; D % 4 == 0 <= 256 (zero-padded columns add nothing), ldx % 4 == 0; 1 <= K <= DIC_MAX_CLUSTERS;
 * N + 256 (K + 2) < 2^30.  medoids (K) int32 row indices, nearest (N) int32, dn / ds (N) f64: all on the DEVICE.  Nothing synchronises `stream`.
 *   dic_kmedoids_workspace / dic_kmedoids_prepare: the split-bf16 planes of the points (centre (D) f32: their column means) in a workspace of
 *       dic_kmedoids_workspace(N, K_max) bytes (16-B aligned), once per fit; K_max = the most slots a pass will take.
 *   dic_kmedoids_assign (exact): for n_rows query rows Q (X itself, or other points: predict) against the K medoid rows of X: nearest, dn, ds and dist
 *       (n_rows, K) f64 = the distance to every medoid (each optional, not all NULL), and td (1) f64 = sum dn in the order above (optional; needs dn).
 *   dic_kmedoids_delta_pass (approximate, on the matrix cores): mode 2 (SWAP): g (N) f64 ~ the first sum of Delta, r (N, K) f64 ~ the second sum per slot,
 *       E (N) f64 with |g[c] + r[c, i] - Delta(c, i)| <= E[c] for every i (also |g - first sum| <= E and |r - second sum| <= E); the derivation stands in
 *       the source file.  mode 1 (BUILD): g ~ g(c) from dn (nearest, ds, r unused).  mode 0 (first BUILD step): g ~ sum_o d(o, c) (dn unused too).
 *       Rows of medoids are computed like any other.  The values are for SELECTING candidates only.
 *   dic_kmedoids_select: v(c) = g[c] + min_{i < cols} r[c, i] (cols = 0: g[c]); U = min over non-medoids of v + E; list (N) int32 receives, in no particular
 *       order, every non-medoid c with v - E <= U, *count (DEVICE int32) their number.  The exact minimum is always among them.
 *   dic_kmedoids_exact: for the M candidates cand[0 .. M-1] (cand NULL: c = 0 .. M-1; count non-NULL: only the first *count (DEVICE) of them) the f64
 *       Delta(c, 0 .. K-1) of the definition into delta (M, K) (mode 2), g(c) into delta (M) (mode 1), sum_o d(o, c) (mode 0), in the order above.
 *       One workgroup of 16 waves works on one candidate at a time; the workgroups stride over the list, and the order of a candidate's sums is the one
 *       stated above whatever the grid.
 *   dic_kmedoids_pick: out (4) f64 DEVICE = {c, i, Delta, entries considered} of the smallest (Delta, c, i) in lexicographic order over delta (M, cols)
 *       (c = -1 when there is none). */
size_t dic_kmedoids_workspace(int64_t N, int K_max);
int dic_kmedoids_prepare(const float* X, long ldx, int64_t N, int D, const float* centre, int K_max, void* workspace, size_t workspace_bytes, dic_stream_t stream);
int dic_kmedoids_assign(const float* Q, long ldq, int64_t n_rows, int D, const float* X, long ldx, int64_t N, const int32_t* medoids, int K, int32_t* nearest,
                        double* dn, double* ds, double* dist, double* td, dic_stream_t stream);
int dic_kmedoids_delta_pass(int64_t N, int K_max, int K, int mode, const int32_t* nearest, const double* dn, const double* ds, double* g, double* r, double* E,
                            void* workspace, size_t workspace_bytes, dic_stream_t stream);
int dic_kmedoids_select(int64_t N, int K_max, int cols, const double* g, const double* r, const double* E, const int32_t* medoids, int n_medoids, int32_t* list,
                        int32_t* count, void* workspace, size_t workspace_bytes, dic_stream_t stream);
int dic_kmedoids_exact(const float* X, long ldx, int64_t N, int D, const int32_t* cand, int64_t M, const int32_t* count, int mode, const int32_t* nearest,
                       const double* dn, const double* ds, int K, double* delta, dic_stream_t stream);
int dic_kmedoids_pick(const int32_t* cand, int64_t M, const int32_t* count, const double* delta, int cols, double* out, dic_stream_t stream);

/* Density-peaks clustering (Rodriguez and Laio, Science 2014; csrc/dic_dpeaks.hip, density_peaks.py), stated here once.
 *   Distances: d(i, j) = sqrt(exact_d2(x_i, x_j)), exact_d2 as csrc/dic_exactd2.h defines it (the f64 difference form of the f32 rows), the root in f64.
 *   Density, one of two:  'cutoff': rho_i = |N_dc(i)| - 1 (an integer), N_dc(i) DBSCAN's neighbour set of eps = d_c, the point itself included
 *       (dic_dbscan_counts with one eps; threshold and band rules unchanged).  'knn': rho_i = 1 / (1 + kth_i / mean(kth)) in f64 on the host, kth_i the
 *       distance to the k-th neighbour, the point itself counted (dic_knn_kth_distance).
 *   Density order: i is denser than j iff rho_i > rho_j, or rho_i == rho_j and i < j: a strict total order; rank_i = i's position in it, rank 0 the densest.
 *   delta and parent: for rank_i > 0, delta_i = min d(i, j) over the denser j, and parent_i = the minimiser of the key (exact_d2(i, j), rank_j): ties in the
 *       exact distance go to the denser point.  For the densest point delta = max_j d(i, j) and parent = -1.  gamma_i = rho_i delta_i.
 *   Centres: n_clusters = K takes the K largest gamma, ties to the smaller rank; or rho_min / delta_min take every point with rho > rho_min and
 *       delta > delta_min, and the densest point is always added.  Cluster ids are 0 .. K-1 in the order of the centres' ranks.
 *   Labels: a centre's root is itself, every other point takes its parent's root (parents have smaller rank: every chain ends).
 *   Halo ('cutoff' only): a border pair is (i, j) with label_i != label_j and j in N_dc(i); border2[c] = max (rho_i + rho_j) over the border pairs with
 *       label_i = c (an integer; 0 when c has none); i is halo iff 2 rho_i < border2[label_i] (strict, as the paper's published code).
 * The kernels take X in DENSITY ORDER (row r = the point of rank r: "denser" is col < row), except dic_dpeaks_border.  X (N, ldx) f32, DEVICE, 16-B aligned,
 * only read; D % 4 == 0 <= 256 (zero-padded columns add nothing), ldx % 4 == 0; 1 <= N < 2^30.  Two calls give the same bits.
 *   dic_dpeaks_workspace / dic_dpeaks_prepare: the split-bf16 planes of the sorted points (centre (D) f32: the f64 column means cast to f32) in a workspace of
 *       dic_dpeaks_workspace(N, D) bytes (16-B aligned); does not synchronise.
 *   dic_dpeaks_delta: on the prepared workspace: delta (N) f64 and parent (N) int32, both DEVICE and in rank space (parent[0] = -1).  cand (capacity, 4)
 *       int32 DEVICE receives the candidate pairs (row, column, the bits of their exact_d2 as two words): every pair the approximate products cannot exclude
 *       from being its row's minimum -- the true minimisers are always among them, and the exact stage alone supplies values and decides ties.  *n_cand (HOST)
 *       = their number; more than `capacity` returns DIC_ERR_WORKSPACE with *n_cand the number needed (nothing written to delta / parent: run again with
 *       capacity >= *n_cand).  stats (2) int64 HOST = {candidates, the longest row's}.  Reads counts back: synchronises `stream`.
 *   dic_dpeaks_border: border2 (n_clusters) int32 DEVICE of the definition from labels (N) int32 in [0, n_clusters) and rho (N) int32, DEVICE, in the
 *       ORIGINAL row order, on the workspace a dic_dbscan_counts call of the same points with the one threshold (the f32 squared-distance threshold of d_c)
 *       left, with its band list (n_band entries, exact masks in .z).  Does not synchronise. */
size_t dic_dpeaks_workspace(int64_t N, int D);
int dic_dpeaks_prepare(const float* X, long ldx, int64_t N, int D, const float* centre, void* workspace, size_t workspace_bytes, dic_stream_t stream);
int dic_dpeaks_delta(const float* X, long ldx, int64_t N, int D, int32_t* cand, int64_t capacity, double* delta, int32_t* parent, int64_t* n_cand,
                     int64_t* stats, void* workspace, size_t workspace_bytes, dic_stream_t stream);
int dic_dpeaks_border(int64_t N, int D, float threshold, const int32_t* labels, const int32_t* rho, int n_clusters, const int32_t* band, int64_t n_band,
                      int32_t* border2, void* workspace, size_t workspace_bytes, dic_stream_t stream);

/* Exact t-SNE in two dimensions (csrc/dic_tsne.hip, tsne.py): sklearn 1.7.2's TSNE(method='exact') on its neighbour-based affinities, stated here once.
 * All arithmetic is f64.
 *   Affinities: k = min(N - 1, int(3 perplexity + 1)); L(i) = the k nearest neighbours of i without i itself (dic_knn_neighbors, self join with k + 1, the
 *       entry of the row's own index dropped, the first entry where it is not among them); r_ij = d_ij^2 - min_j d_ij^2.  beta_i is found by sklearn's
 *       search: beta = 1, no bounds; per step p_j = exp(-beta r_ij), s = sum p, H = log s + beta (sum r p) / s; stop if |H - log perplexity| <= 1e-10 or
 *       at the 200th evaluation; else H too large: lower bound = beta and beta doubles while there is no upper bound, else the midpoint; H too small: upper
 *       bound = beta and beta halves while there is no lower bound, else the midpoint.  p_j|i = p_j / s and beta_i are those of the LAST evaluation (a
 *       row whose nearest entries are all at distance 0 and the step cap end there).  P_ij = (p_j|i + p_i|j) / sum over all pairs of the same.
 *   Map: Y (N, 2).  q_ij = 1 / (1 + |y_i - y_j|^2) for i != j, Z = sum_{i != j} q_ij, Q = q / Z.  With the exaggeration e:
 *       grad_i = 4 (sum_j e P_ij q_ij (y_i - y_j) - (sum_{j != i} q_ij^2 (y_i - y_j)) / Z);  KL = e (sum P log P + log e + sum P log(1 + d^2) + log Z).
 *   Update (sklearn's _gradient_descent): gains += 0.2 where update * grad < 0, else *= 0.8; gains >= 0.01; update = momentum update - lr (grad gains);
 *       Y += update.  250 iterations at e = early_exaggeration and momentum 0.5, then e = 1 and momentum 0.8; the checks run every 50 iterations.
 * Everything is on the DEVICE; no floating-point atomics; two calls give the same bits; nothing synchronises `stream`.  2 <= N < 2^30.
 *   dic_tsne_perplexity: d2 (M, k) row-major = r (the row minimum already subtracted), 1 <= k <= 1024, perplexity > 0: beta (M) and p (M, k) OVERWRITTEN.
 *       One wave per row; the sums of a step are per-lane sums over the entries lane, lane + 64, .. ascending, then the xor tree 32, 16, .., 1.
 *   dic_tsne_repulsion: for the map Y (N, 2), 16-B aligned, leaves in the workspace (dic_tsne_repulsion_workspace(N) bytes, 16-B aligned): Z at double 0,
 *       and behind it, per column split s < S = dic_tsne_splits(N), the partial sums over the split's columns of q^2 (y_i - y_j) (x, y) and of q.  The
 *       splits, the 256-column chunks and the 64-column piece each of the four waves takes are functions of N alone; a wave adds its columns in ascending
 *       order, the four waves are added in wave order, the splits in split order by the consumer.  1 / (1 + d^2) is an f32 reciprocal refined by two f64
 *       Newton steps (relative error of a few 2^-53).  The pair (i, i) and the padding of the last block contribute exactly nothing.  |y| < 1e18.
 *   dic_tsne_step: on that workspace and the symmetric CSR of P (indptr (N + 1) int64, indices (nnz) int32, pval (nnz) f64; an entry outside [0, N) is
 *       absent, indptr is clamped to [0, nnz]): the gradient of the definition -- per row the lane sums over entries lane, lane + 64, .. ascending by fma,
 *       then the xor tree -- written to grad (N, 2) (optional), and with update, gains (N, 2, IN/OUT) and Ynew (N, 2, OVERWRITTEN, never Y) non-NULL the
 *       update rule: Ynew = Y + update.  All three NULL: the gradient alone.  partials (dic_tsne_step_partials(N), 2) OVERWRITTEN: per workgroup of four
 *       rows the sums of |grad_i|^2 and of sum_j P_ij log(1 + d_ij^2) in row order; the host adds them when it checks progress. */
int dic_tsne_perplexity(const double* d2, int64_t M, int k, double perplexity, double* beta, double* p, dic_stream_t stream);
int dic_tsne_splits(int64_t N);
size_t dic_tsne_repulsion_workspace(int64_t N);
int dic_tsne_repulsion(const double* Y, int64_t N, void* workspace, size_t workspace_bytes, dic_stream_t stream);
int64_t dic_tsne_step_partials(int64_t N);
int dic_tsne_step(const int64_t* indptr, const int32_t* indices, const double* pval, int64_t N, int64_t nnz, const double* Y, const void* workspace,
                  size_t workspace_bytes, double exaggeration, double momentum, double learning_rate, double* update, double* gains, double* Ynew,
                  double* grad, double* partials, dic_stream_t stream);

/* Local outlier factor (csrc/dic_lof.hip, lof.py): sklearn 1.7.2's LocalOutlierFactor for the euclidean metric, stated here once.  All arithmetic is f64.
 *   A fit on N rows uses k = max(1, min(n_neighbors, N - 1)).  (dist, idx) (N, k): the k nearest rows of every row sorted by (distance, index), its own index
 *       left out (dic_knn_neighbors, self join with k + 1, the entry of the row's own index dropped, the first entry where it is not among them).
 *       kdist[j] = dist[j, k - 1];  reach(i, s) = max(kdist[idx[i, s]], dist[i, s]);  lrd[i] = 1 / (mean_s reach(i, s) + 1e-10);
 *       negative_outlier_factor[i] = -mean_s (lrd[idx[i, s]] / lrd[i]).
 *   New rows (novelty): (dist, idx) (M, k) are their k nearest rows of the fitted set, nothing left out; kdist and the neighbours' lrd are the fit's, lrd_q
 *       is formed as above, score = -mean_s (lrd[idx[q, s]] / lrd_q[q]).
 *   Several k from one set of lists: the first k columns of a (distance, index)-ordered list are the list at k, so every k is defined on a prefix.
 * ks (nk) int HOST, strictly ascending, 1 <= ks[t] <= ld, 1 <= nk <= 64 (more: DIC_ERR_UNSUPPORTED).  dist (M, ld) f64 and idx (M, ld) int32 row-major with
 * row stride ld, DEVICE; the tables kdist, lrd_fit (n, nk) and lrd, lrd_rows, nof (M, nk) f64 DEVICE, column t belonging to ks[t].  1 <= M, n < 2^30.  The
 * CONTENTS of idx are not validated: the caller guarantees 0 <= idx < n (an entry outside is clamped into the range -- no wild read, a meaningless value).
 * Every sum runs over s = 0 .. ks[t] - 1 in that order, whatever the launch geometry and the other entries of ks: no floating-point atomics, two calls give the
 * same bits, and column t of a call with several k has the bits of the call with ks[t] alone.  Nothing synchronises `stream`.
 *   dic_lof_lrd: lrd[i, t] = 1 / ((sum_{s < ks[t]} max(kdist[idx[i, s], t], dist[i, s])) / ks[t] + 1e-10), OVERWRITTEN.  For the fit M = n and the lists are
 *       the self-excluded ones.
 *   dic_lof_scores: nof[i, t] = -(sum_{s < ks[t]} lrd_fit[idx[i, s], t]) / (ks[t] lrd_rows[i, t]), OVERWRITTEN (the fit: lrd_rows = lrd_fit). */
int dic_lof_lrd(const double* dist, const int32_t* idx, int64_t M, int ld, const double* kdist, int64_t n, const int* ks, int nk, double* lrd,
                dic_stream_t stream);
int dic_lof_scores(const int32_t* idx, int64_t M, int ld, const double* lrd_fit, int64_t n, const double* lrd_rows, const int* ks, int nk, double* nof,
                   dic_stream_t stream);

/* DBCV, Density-Based Clustering Validation (Moulavi, Jaskowiak, Campello, Zimek, Sander, SDM 2014; csrc/dic_dbcv.hip, dbcv.py), stated here once.
 *   Inputs: points X (N, D <= 256) f32; labels, -1 for noise, any other ids; dpow, the number of features used as the exponent (the caller's column count,
 *       not the padded D).  d(o, p) is the f64 difference-form distance of the f32 coordinates.  A cluster with one member is treated as noise: it contributes
 *       0 and counts in N.  Fewer than two remaining clusters: an error of the caller.
 *   All-points core distance of o in cluster C (n = |C| >= 2), over the other members p of C with d(o, p) > 0 (coincident members are skipped):
 *       m = the smallest such distance;  S = sum_p (m / d(o, p))^dpow, each term formed as exp(dpow / 2 * log(m^2 / d^2(o, p)));
 *       a(o) = m (S / (n - 1))^(-1 / dpow);  a(o) = 0 where no member lies at a nonzero distance.
 *       (The paper's (sum (1 / d)^dpow / (n - 1))^(-1 / dpow) with the largest term factored out: every term lies in (0, 1], nothing leaves f64's range.)
 *   Within a cluster: mr(o, p) = max(a(o), a(p), d(o, p)).  The spanning tree is the one dic_hdbscan_mst walks over the cluster's members in ascending row
 *       order from its first member with core = a (ties: the smallest index).  Internal nodes: tree degree >= 2; none: the first member.  Internal edges:
 *       both ends internal; none: all edges.  DSC(C) = the largest internal edge weight.
 *   Between clusters: sep(C) = min over internal o in C and internal p of any other (non-noise, non-singleton) cluster of max(a(o), a(p), d(o, p)).
 *       V(C) = (sep - DSC) / max(sep, DSC), 0 where both are 0.  DBCV = sum_C |C| / N V(C), N counting every row, noise included.
 * Both entry points take the rows SORTED by (cluster, row), noise and singletons left out by the caller: X (N, D) f32 DEVICE, row stride ldx floats, D % 4 == 0,
 * ldx % 4 == 0, 16-B aligned (zero columns change nothing), 1 <= N < 2^30; seg_start (K + 1) int32 DEVICE, ascending, seg_start[0] = 0, seg_start[K] = N:
 * segment s is rows seg_start[s] .. seg_start[s + 1] - 1, 1 <= K <= N.  The CONTENTS of seg_start are not validated (no wild access whatever they are).
 * workspace: dic_dbcv_workspace(N, K) bytes DEVICE, 16-B aligned, no state between calls.  A pair's d^2 is one f64 fma chain over the coordinates in order
 * 0 .. D - 1.  No floating-point atomics; two calls give the same bits, whatever the launch geometry.  Nothing synchronises `stream`.
 *   dic_dbcv_core: a (N) f64 OVERWRITTEN, as defined above; only pairs inside a segment are touched.  1 <= dpow <= 65536.  Terms of S below e^-60 are left
 *       out (fewer than 2^30 of them against S >= 1: a moves by less than 1e-17 / dpow relatively).
 *   dic_dbcv_separation: a (N) f64 and internal (N) uint8 (nonzero: the row is an internal node) in; rowsep (N) f64 and rowarg (N) int32 OVERWRITTEN:
 *       rowsep[o] = min over flagged rows p of OTHER segments of max(a[o], a[p], d(o, p)) and rowarg[o] the p that attains it, the smallest among equals; a
 *       row with no flagged row in another segment gets +inf and -1.  Every row o gets a value, flagged or not.  The flagged rows are first gathered into
 *       an ascending list in the workspace and only they are walked as columns: the pass costs N x #flagged pairs. */
size_t dic_dbcv_workspace(int64_t N, int64_t K);
int dic_dbcv_core(const float* X, long ldx, int64_t N, int D, const int32_t* seg_start, int64_t K, double dpow, double* a, void* workspace,
                  size_t workspace_bytes, dic_stream_t stream);
int dic_dbcv_separation(const float* X, long ldx, int64_t N, int D, const int32_t* seg_start, int64_t K, const double* a, const unsigned char* internal,
                        double* rowsep, int32_t* rowarg, void* workspace, size_t workspace_bytes, dic_stream_t stream);

/* Agreement of two labellings a, b of the same N rows (csrc/dic_agreement.hip, agreement.py): sklearn 1.7.2's sklearn.metrics.cluster, stated here once, for
 * P pairs of the L rows of one code matrix in one launch per stage.
 *   Inputs: codes (L, N) int32 DEVICE, row stride ld: row l holds the class of every row of the data under labelling l as a code in [0, K_l) (the caller
 *       encodes; -1 is a class like any other).  drop (L) int32 DEVICE or NULL: a row whose code under EITHER labelling of a pair equals that labelling's
 *       drop[l] is left out of the pair (-1: nothing to drop).  A code outside [0, K_l) is skipped: no wild access.
 *   desc (P, 8) int64 DEVICE, one row per pair: {la, lb, Ka, Kb, table_off, marg_off, part_off, 0}: the pair's table n (Ka, Kb) int32 row-major starts at
 *       tables + table_off, its marginals a (Ka) then b (Kb) int64 at marg + marg_off, its Ka * ceil(Kb / 64) EMI partials at double word part_off of the
 *       workspace.  A pair whose descriptor points outside a buffer (total_cells, total_marg, the workspace) or has la, lb outside [0, L) is SKIPPED by
 *       every stage and its outputs are left as they were.  1 <= L, P < 2^24; N < 2^31.
 *   Per pair: n_ij = #{r : a_r = i, b_r = j};  a_i = sum_j n_ij;  b_j = sum_i n_ij;  N' = sum_ij n_ij (the rows counted: N without drop).
 *       isums = {sum_ij n_ij^2, sum_i a_i^2, sum_j b_j^2, N'} int64.  (Pair confusion, Rand, ARI and FMI are integer expressions of these: agreement.py.)
 *       MI = sum over the cells with n_ij > 0 of t_ij, in f64 with sklearn's grouping (cnm = n_ij / N', every log of the integer converted to f64,
 *           a_i * b_j formed in int64):
 *               t_ij = cnm * (log(n_ij) - log(N')) + cnm * ((-log(a_i * b_j) + log(N')) + log(N')),  set to 0 where |t_ij| < 2^-52;
 *           no fused multiply-add.  ORDER: thread t of 256 adds the cells c = t, t + 256, .. of the row-major table in ascending order, starting from 0; the
 *           256 sums are then added by a binary tree, x[t] += x[t + s] for s = 128, 64, .., 1.
 *       H(a) = -sum_{a_i > 0} (a_i / N') * (log(a_i) - log(N')), thread t adding i = t, t + 256, .., then the same tree and one negation; H(b) likewise.
 *       EMI = sum over ALL cells (i, j) with a_i, b_j > 0 and n = max(1, a_i + b_j - N') .. min(a_i, b_j) of
 *               ((n / N') * (((log(N') + log(n)) - log(a_i)) - log(b_j))) * exp(g),  with lf[m] = ln m! the CALLER's table (lf_len >= N' + 1 doubles) and
 *               g = ((((((lf[a_i] + lf[b_j]) + lf[N' - a_i]) + lf[N' - b_j]) - (lf[n] + lf[N'])) - lf[a_i - n]) - lf[b_j - n]) - lf[N' - a_i - b_j + n]
 *           -- sklearn's order of the nine terms.  Terms with g < -746 are left out: exp is exactly 0 there, no bit changes.
 *           ORDER: a unit u = i * ceil(Kb / 64) + c is row i and the columns j = 64 c .. 64 c + 63 of the table, summed by the 64 lanes of one wave, each
 *           lane from 0: where a_i <= 32, lane l takes column 64 c + l and adds its n ascending; else the columns are taken in ascending order and within one
 *           lane l adds n = lo + l, lo + l + 64, ..  The 64 lane sums are added by the butterfly x += x[lane ^ m], m = 32, 16, .., 1, which gives the unit's
 *           partial.  Thread t of 256 adds the partials u = t, t + 256, .. ascending, then the binary tree above.
 *   Integer adds commute (integer LDS / global atomics only), no floating-point atomics: two calls give the same bits, and a pair's results do not depend on
 *   which other pairs share the call.  Nothing synchronises `stream`.
 *   dic_agreement_lds_cells: the largest table (Ka * Kb cells) that is counted in LDS and flushed once per workgroup; a larger one is counted in global memory.
 *   dic_agreement_workspace(total_units): bytes DEVICE, 16-B aligned, for the EMI partials of all pairs (total_units = sum over pairs of Ka * ceil(Kb / 64)).
 *   dic_agreement_tables: tables (total_cells) int32 OVERWRITTEN (zeroed, then counted).
 *   dic_agreement_sums: marg (total_marg) int64, isums (P, 4) int64 and fsums (P, 3) f64 = {MI, H(a), H(b)} OVERWRITTEN for every pair that is not skipped.
 *   dic_agreement_emi: marg and isums as dic_agreement_sums left them; max_units the largest Ka * ceil(Kb / 64) of the pairs (< 2^26); emi (P) f64
 *       OVERWRITTEN.  A pair with N' >= lf_len gets NaN. */
int dic_agreement_lds_cells(void);
size_t dic_agreement_workspace(int64_t total_units);
int dic_agreement_tables(const int32_t* codes, int64_t ld, int64_t L, int64_t N, const int32_t* drop, const int64_t* desc, int64_t P, int32_t* tables,
                         int64_t total_cells, dic_stream_t stream);
int dic_agreement_sums(const int32_t* tables, int64_t total_cells, const int64_t* desc, int64_t L, int64_t P, int64_t* marg, int64_t total_marg,
                       int64_t* isums, double* fsums, dic_stream_t stream);
int dic_agreement_emi(const int64_t* marg, int64_t total_marg, const int64_t* desc, int64_t L, int64_t P, int64_t max_units, const int64_t* isums,
                      const double* lf, int64_t lf_len, double* emi, void* workspace, size_t workspace_bytes, dic_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DIC_HIP_H */

/* nvit_hip.h — C ABI of the MI355X (gfx950) nViT hot-path library (libnvit_hip.so).
 *
 * Drop-in boundary: the reference has no FFI; its seams are the Python
 * classes in /root/reference/nvit/model.py and Trainer.normalize_matrices
 * (/root/reference/nvit/train.py:461-480).  Every entry point below replaces the torch
 * operator sequence cited next to it.  Conventions:
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless marked host;
 *   - the caller owns every buffer (outputs, workspaces, saved-for-backward tensors);
 *     the library never allocates, frees or keeps a pointer past the call;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); calls are
 *     asynchronous and re-entrant (forward on the main thread, backward on the autograd
 *     thread); the only global state is the optional event-timing table (nvit_prof_*);
 *   - return 0 on success, NVIT_EINVAL for a rejected argument, else a hipError_t value;
 *     nvit_last_error() gives the calling thread's message.  No exception crosses the ABI.
 *   - `dt` selects the activation / MFMA-operand type: NVIT_F32 (exact-f32 MFMA path,
 *     parity <=1e-5) or NVIT_BF16 (bf16 operands, fp32 accumulate).  The residual stream,
 *     parameters, gradients and all reductions are fp32 in both modes.
 *   - token-major activations are [M, C] with M = B*T rows; per-head tensors are
 *     [B, H, T, d] contiguous.
 *   - Python binds from this text (nvit_amd/_lib.py), so a prototype is written `<return> nvit_<name>(<type> <name>, ...);`
 *     outside comments: every parameter named; pointers, int, unsigned, int64_t, uint64_t, float, double; returns of
 *     those, void or const char*.  Anything else fails the import.
 */
#ifndef NVIT_HIP_H
#define NVIT_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NVIT_OK 0
#define NVIT_EINVAL 1001
#define NVIT_F32 0
#define NVIT_BF16 1
#define NVIT_BF16_F32IN 3 /* nvit_qknorm_fwd / nvit_swiglu_fwd only: fp32 inputs (unrounded GEMM outputs), bf16 outputs */

int nvit_version(void);
const char* nvit_last_error(void);

/* ---- event timing of kernel families (bench.py roofline leg) ------------------ */
#define NVIT_KID_GEMM_NT 0
#define NVIT_KID_GEMM_TN 1
#define NVIT_KID_ATTN_FWD 2
#define NVIT_KID_ATTN_BWD 3
#define NVIT_KID_ROWOPS 4
#define NVIT_KID_RENORM 5
#define NVIT_KID_SHADOW 6
#define NVIT_KID_PATCHIFY 7
#define NVIT_KID_MISC 8
#define NVIT_KID_GEMM_F32 9 /* exact-f32 MFMA GEMMs (fp32 mode; patch embedding + classifier of the bf16 mode) */
#define NVIT_KID_GEMM_SWIGLU 10     /* bf16 NT GEMM with the SwiGLU epilogue (nvit_gemm_nt_swiglu) */
#define NVIT_KID_GEMM_QKNORM 11     /* bf16 NT GEMM with the q/k-normalise + head-split epilogue (nvit_gemm_nt_qknorm) */
#define NVIT_KID_GEMM_SWIGLU_BWD 12 /* bf16 NT GEMM with the SwiGLU-backward epilogue (nvit_gemm_nt_swiglu_bwd) */
#define NVIT_KID_OPTIM 13           /* nvit_grad_sqnorm + nvit_adamw_renorm (NVIT_KID_RENORM = stand-alone nvit_renorm_weights) */
#define NVIT_KID_GEMM_SWIGLU_ACT 14 /* bf16 NT GEMM with the gate-only SwiGLU epilogue (nvit_gemm_nt_swiglu_act) */
#define NVIT_KID_COUNT 15
void nvit_prof_enable(int on);
/* time only the families whose bit is set (bit k = family k of nvit_prof_name); nvit_prof_enable(1) = all, (0) = none */
void nvit_prof_select(unsigned mask);
/* Synchronises the recorded events and returns, per kernel family, total milliseconds,
 * algorithmic FLOPs, algorithmic bytes and launch count since the last collect. Host arrays
 * of NVIT_KID_COUNT entries. */
int nvit_prof_collect(double* ms, double* flops, double* bytes, int64_t* launches);
const char* nvit_prof_name(int kid);

/* ---- weights --------------------------------------------------------------------
 * nvit_renorm_weights: Trainer.normalize_matrices (train.py:461-480) as ONE persistent
 * launch.  `table` is a device array of n rows of 5 int64: {ptr, rows, cols, dim, first_item}
 * dim=1: every row scaled to unit L2 norm (query/key/value/c_fc); dim=0: every column
 * (att_c_proj/mlp_c_proj).  fp32 in place, one read + one write per element.
 * first_item = prefix sum of work items (rows/NVIT_RENORM_ROWS_PER_ITEM for dim=1,
 * cols/NVIT_RENORM_COLS_PER_ITEM for dim=0, rounded up; cols/NVIT_RENORM_TALL_COLS_PER_ITEM for a dim=0 matrix of
 * more than NVIT_RENORM_TALL_ROWS rows); total_items = sum.
 * dim=0 keeps a [rows x NVIT_RENORM_COLS_PER_ITEM] panel in the registers of a 1024-thread workgroup (rows <=
 * NVIT_RENORM_TALL_ROWS), a [rows x NVIT_RENORM_TALL_COLS_PER_ITEM] panel for taller matrices of up to
 * NVIT_RENORM_MAX_ROWS_DIM0 rows.  dim=1 takes any number of columns (rows of up to NVIT_MAX_EMBD columns, a multiple of
 * 4, stay in registers). */
#define NVIT_RENORM_ROWS_PER_ITEM 64
#define NVIT_RENORM_COLS_PER_ITEM 64
#define NVIT_RENORM_TALL_ROWS 1152          /* dim=0 matrices with more rows take the narrow panel */
#define NVIT_RENORM_TALL_COLS_PER_ITEM 32
#define NVIT_RENORM_MAX_ROWS_DIM0 2048
#define NVIT_RENORM_MAX_GRID 2048           /* workgroups of the launch: workgroup b takes the items b, b + grid, ... */
int nvit_renorm_weights(const int64_t* table, int n, int total_items, void* stream);

/* nvit_shadow_weights: builds the private MFMA-operand copies of the fp32 master weights
 * (SURVEY.md §8b "state_dict contract": non-persistent shadows) in ONE launch.  `table` =
 * device array of n rows of 12 int64:
 *   {src, rows, cols, dst, dst_ld, dst_cols, dstT, dstT_ld, dstT_cols, perm, first_item, tiles_c}
 *   dst  [rows, dst_ld]  : dst[r, c] = src[perm(r), c] for c < cols, 0 for cols <= c < dst_cols
 *   dstT [cols, dstT_ld] : dstT[c, r] = dst[r, c] for r < rows, 0 for rows <= r < dstT_cols
 *   Either dst or dstT may be 0 (skipped).  dst/dstT may point inside a larger concatenated
 *   buffer (Q|K|V stacking); only the stated extents are written.
 *   perm: 0 identity; 1 = SwiGLU interleave of a [2F, K] matrix: shadow row 32q+w is
 *         source row 16q+w (w<16, "u") or F+16q+(w-16) (w>=16, "v");
 *         2 = split-precision image (dt = bf16 only, dstT unused): dst [rows, 2*Kp], Kp = nvit_patch_embed_kp(cols);
 *         columns 32j..32j+31 of src become the 128-byte slice [hi32 | lo32] at dst column 64j, hi = bf16(src),
 *         lo = bf16(src - hi) - the weight operand of nvit_patch_embed_fwd.  The padding columns of the last
 *         slice are NOT written: allocate dst zeroed.
 *   Work items are square tiles of NVIT_SHADOW_TILE elements a side: tiles_c = ceil(max(cols,dst_cols)/NVIT_SHADOW_TILE)
 *   tile columns, ceil(max(rows,dstT_cols)/NVIT_SHADOW_TILE) tile rows; first_item = prefix sum; total_items = sum.
 * Element type of dst/dstT is `dt`. */
#define NVIT_SHADOW_TILE 64
int nvit_shadow_weights(const int64_t* table, int n, int total_items, int dt, void* stream);

/* Optimizer step fused with the re-normalisation: replaces clip_grad_norm_ + AdamW.step +
 * Trainer.normalize_matrices (train.py:935-946, 461-480, 989-990; parameter groups of model.py:369-385).
 * table: n rows of NVIT_OPT_TABLE_COLS int64 {p, g, m, v (fp32 device pointers), rows, cols, kind, first_item,
 *        first_chunk, f32bits(lr) | f32bits(weight_decay) << 32};  kind -1 = plain (items of NVIT_OPT_CHUNK elements),
 *        1 = normalise rows (items of NVIT_OPT_ROWS_PER_ITEM rows; cols % 4 == 0, cols <= NVIT_OPT_WIDE_COLS), 0 =
 *        normalise columns (rows <= NVIT_OPT_TALL_ROWS; items of NVIT_OPT_SLAB_COLS columns, of NVIT_OPT_TALL_COLS
 *        columns for a matrix of more than NVIT_OPT_SLAB_ROWS rows);
 *        first_chunk counts NVIT_OPT_CHUNK-element chunks of the gradient for nvit_grad_sqnorm.
 * nvit_grad_sqnorm: partial[npart] = per-workgroup sums of g*g over all gradients (npart <= NVIT_OPT_MAX_PART
 *        workgroups).
 * nvit_adamw_renorm: clip = min(1, max_norm / (sqrt(sum partial) + 1e-6)) when partial != NULL and max_norm > 0;
 *        g *= clip; torch AdamW update (decoupled decay, bias corrections 1 - beta^t passed by the host); rows /
 *        columns of kind 1 / 0 matrices are L2-normalised before the single write-back.  gnorm_out[0] (optional)
 *        receives the pre-clip global gradient norm.  max_slab_rows sizes the LDS: the largest `rows` among kind-0
 *        entries, and at least NVIT_OPT_WIDE_LDS_ROWS when a kind-1 entry has more than NVIT_OPT_ROW_COLS columns (such
 *        rows are parked in LDS).
 *        hyper (optional, 3 floats on the device): when given, the bias corrections are read from hyper[1..2] as
 *        maintained by nvit_adamw_tick (hyper[0] = step count; one call per optimizer step, before this one), so the
 *        whole step can be captured in a hipGraph and replayed; the two double arguments are then ignored. */
#define NVIT_OPT_TABLE_COLS 10
#define NVIT_OPT_CHUNK 8192          /* elements per plain item and per grad-norm chunk */
#define NVIT_OPT_ROWS_PER_ITEM 16
#define NVIT_OPT_SLAB_COLS 32        /* column slab of a kind-0 matrix of at most NVIT_OPT_SLAB_ROWS rows, */
#define NVIT_OPT_SLAB_ROWS 1152
#define NVIT_OPT_TALL_COLS 16        /* of a taller one (at most NVIT_OPT_TALL_ROWS rows) */
#define NVIT_OPT_TALL_ROWS 2048
#define NVIT_OPT_ROW_COLS 1536       /* a kind-1 row of at most this many columns stays in registers, */
#define NVIT_OPT_WIDE_COLS 2048      /* a wider one (up to this) is parked in LDS, */
#define NVIT_OPT_WIDE_LDS_ROWS 1024  /* which is then sized as for a slab of this many rows */
#define NVIT_OPT_MAX_PART 4096
#define NVIT_OPT_MAX_GRID 2048       /* workgroups of nvit_adamw_renorm: workgroup b takes the items b, b + grid, ... */
int nvit_adamw_tick(float* hyper, double beta1, double beta2, void* stream);
int nvit_grad_sqnorm(const int64_t* table, int n, int total_chunks, float* partial, int npart, void* stream);
int nvit_adamw_renorm(const int64_t* table, int n, int total_items, int max_slab_rows, float beta1, float beta2,
                      float eps, double bias_correction1, double bias_correction2, const float* partial, int npart,
                      float max_norm, float* gnorm_out, const float* hyper, void* stream);
/* The same step, left out when the gradients are not finite (GradScaler.step of the reference, train.py:930-942).
 * Order: nvit_grad_sqnorm, nvit_adamw_tick_guarded, nvit_adamw_renorm_guarded.
 * skip_state: 2 floats on the device, zeroed by the caller once: {the last step was skipped (0 / 1), steps skipped}.
 * nvit_adamw_tick_guarded: one workgroup sums partial[npart] and decides for the whole step.  Finite sum: hyper[0..2]
 *        advance as in nvit_adamw_tick and skip_state[0] = 0.  Inf or NaN (also a squared norm that overflows fp32):
 *        hyper is left alone, skip_state[0] = 1, skip_state[1] += 1.
 * nvit_adamw_renorm_guarded: nvit_adamw_renorm with partial, gnorm_out and hyper required; gnorm_out[0] is always
 *        stored (max_norm = 0 switches the clipping off, not the norm); then every workgroup reads skip_state[0] and
 *        returns when it is set, so p, m and v stay bit-identical.  An applied step gives the bits of nvit_adamw_renorm. */
int nvit_adamw_tick_guarded(float* hyper, double beta1, double beta2, const float* partial, int npart,
                            float* skip_state, void* stream);
int nvit_adamw_renorm_guarded(const int64_t* table, int n, int total_items, int max_slab_rows, float beta1, float beta2,
                              float eps, const float* partial, int npart, float max_norm, float* gnorm_out,
                              const float* hyper, const float* skip_state, void* stream);
/* Learning-rate schedule on the device (LRSchedule): one workgroup of NVIT_LR_SCHEDULE_THREADS threads, once per
 * optimizer step, after the table is in place and before nvit_grad_sqnorm / nvit_adamw_renorm*.  With s = step[0] (an
 * int64 on the device, optimizer steps attempted so far), W = warmup_iters, D = decay_iters, all converted to double:
 *        s <  W : L = warmup_init + (lr - warmup_init) * s / W
 *        else, kind NVIT_LR_CONSTANT: L = lr (D is ignored)
 *        s >  D : L = min_lr
 *        else   : r = (s - W) / (D - W);  NVIT_LR_COSINE: L = min_lr + (0.5 * (1.0 + cos(pi * r))) * (lr - min_lr),
 *                 NVIT_LR_LINEAR: L = lr + (min_lr - lr) * r
 *        in fp64, in this operation order, without fused multiply-adds (the trainer's get_lr, train.py:1025-1035, for
 *        kind NVIT_LR_COSINE and warmup_init = 0).  Then step[0] = s + 1, last_lr[0] = (float)L, last_lr64[0] = L, and row
 *        i of the table (the one of nvit_adamw_renorm; n rows, n == 0 with table == NULL only advances the counter)
 *        receives (float)(L * (double)lr_scale[i]) in the lr half of its last column; its weight_decay half and all
 *        other columns stay as they are.  Needs W >= 0, D > W unless the kind is constant, finite rates >= 0. */
#define NVIT_LR_COSINE 0
#define NVIT_LR_LINEAR 1
#define NVIT_LR_CONSTANT 2
#define NVIT_LR_SCHEDULE_THREADS 256
int nvit_lr_schedule(int64_t* table, int n, const float* lr_scale, int64_t* step, int kind, double lr, double min_lr,
                     double warmup_init, int64_t warmup_iters, int64_t decay_iters, float* last_lr, double* last_lr64,
                     void* stream);

/* Exponential moving average of the weights (ModelEma), two launches per optimizer step: nvit_ema_tick, nvit_ema_update.
 * state: 4 floats on the device, zeroed by the caller once: {t = updates applied so far, omd = 1 - d of the update about
 *        to run, spare, spare}.  The count is a float, exact up to 2^24 updates, like hyper[0] of nvit_adamw_tick.
 * nvit_ema_tick: one thread, in fp64: d = warmup ? min(decay, (1 + t) / (10 + t)) : decay with t the count before this
 *        update; stores omd = (float)(1 - d) and t + 1.  skip_state (optional, the optimizer's own): when given and
 *        skip_state[0] != 0 the count stays as it is and omd = 0 is stored.
 * nvit_ema_update: table = n rows of NVIT_EMA_TABLE_COLS int64 {src, dst (fp32 device pointers), numel, first_chunk,
 *        flags}; work items are chunks of NVIT_EMA_CHUNK elements, first_chunk = prefix sum, total_chunks = sum; at most
 *        NVIT_EMA_MAX_GRID workgroups, workgroup b takes the chunks b, b + grid, ...  Per element dst = fma(omd, src -
 *        dst, dst) with omd = state[1]; every workgroup returns before it touches memory when omd == 0.  A row with
 *        NVIT_EMA_FLAG_COPY stores src unchanged.  A row whose numel is no multiple of 4, or whose src or dst is not
 *        16-byte aligned, must carry NVIT_EMA_FLAG_SCALAR (element-wise accesses; the others use float4).  The src and
 *        dst ranges of a table must not overlap.  state == NULL: only the copy rows run. */
#define NVIT_EMA_TABLE_COLS 5
#define NVIT_EMA_CHUNK 4096
#define NVIT_EMA_MAX_GRID 2048
#define NVIT_EMA_FLAG_COPY 1
#define NVIT_EMA_FLAG_SCALAR 2
int nvit_ema_tick(float* state, double decay, int warmup, const float* skip_state, void* stream);
int nvit_ema_update(const int64_t* table, int n, int total_chunks, const float* state, void* stream);

/* ---- GEMMs ------------------------------------------------------------------------
 * nvit_gemm_nt: C[M,N] = A[M,K] * B[N,K]^T  (nn.Linear: model.py:99-101,130,148,155,...)
 * A, B of type dt, K % (128/sizeof(dt)) == 0, lda/ldb multiples of 16 bytes.
 * Epilogue, in this order: +bias[n]; *colscale[n]; +rowadd[(m % rowadd_period)*N + n];
 * + old C (accumulate!=0); store as out_dt (NVIT_F32 / NVIT_BF16) with leading dim ldc. */
int nvit_gemm_nt(int dt, const void* A, int lda, const void* B, int ldb, void* C, int ldc, int out_dt,
                 int M, int N, int K, const float* bias, const float* colscale, const float* rowadd,
                 int rowadd_period, int accumulate, void* stream);

/* Fused-epilogue variants of nvit_gemm_nt (bf16 operands; N % 256 == 0, K % 64 == 0 — query with
 * nvit_gemm_nt_fusable; otherwise callers run nvit_gemm_nt followed by nvit_swiglu_fwd / nvit_qknorm_fwd).
 * nvit_gemm_nt_swiglu: uv[M,2F] = A B^T with B the perm=1 (u16|v16 interleaved) shadow of c_fc / proj, AND
 *   xm[M,F] = (gu*u)*silu(gv*v), gu/gv = gs[.]*gscale with gs = suv in the same interleaved order (NULL = 1)
 *   (model.py:148-154: the [M,8C] pre-activation is written once, never re-read in forward).
 * nvit_gemm_nt_qknorm: q/k/v projections (nparts stacked [C,K] weights starting at part part0: 0=q,1=k,2=v) with
 *   the per-head L2 normalise, sqk*c_q scale and [B,H,T,64] head split done on the fp32 accumulators
 *   (model.py:99-119); rq/rk [M,H] = 1/||.||.  Requires head dim 64 and n_embd % 256 == 0.
 *   sqk == NULL: the head split alone (plain-ViT attention, model.py:97-100): no normalise, q multiplied by
 *   q_prescale only, k and v stored as they are; rq, rk and c_q are not used.
 * nvit_gemm_nt_swiglu_bwd: autograd of model.py:148-155 / 259-262 in one launch: dx[M,F] = A B^T (A = dL/dy of
 *   mlp_c_proj / out_proj, B = that weight's transposed shadow [F,K]) stays in the accumulators; with the saved raw
 *   uv[M,2F] (interleaved, as written by nvit_gemm_nt_swiglu) it writes duv[M,2F] (same layout) and, when gs != NULL
 *   (suv, natural order [u(F)|v(F)]), part[R, 2F] = partial sums of d(suv) over NVIT_SWIGLU_BWD_PART_ROWS rows each, for
 *   whole row tiles: R = ceil(M / NVIT_SWIGLU_BWD_TILE_ROWS) * NVIT_SWIGLU_BWD_TILE_ROWS / NVIT_SWIGLU_BWD_PART_ROWS (natural
 *   order; reduce with nvit_colsum_reduce).  Replaces nvit_gemm_nt + nvit_swiglu_bwd.  Requires F % 256 == 0.
 * bias (optional) of the three forward forms: fp32, 16-byte aligned, NULL = none.  bias[n] is added to the fp32 accumulator
 * of output column n FIRST, before anything else in the epilogue, so every later step sees A B^T + bias:
 *   _swiglu / _swiglu_act: bias[2F] in the interleaved (perm=1, u16|v16) column order of the weight shadow, like gs.  The
 *     raw uv that is stored (the pre-activation nvit_gemm_nt_swiglu_bwd / nvit_swiglu_bwd differentiate) includes it, and
 *     the gate is computed from the same biased sums: xm of the two forms stays bit-identical.
 *   _qknorm: bias[nparts*C], the stacked biases of exactly the nparts projections of this launch, indexed by the launch's
 *     own output column (NOT offset by part0).  Added for every part (v too) before the sum of squares; the normalise,
 *     rq/rk, the sqk*c_q scale, q_prescale and the head split (also with sqk == NULL) run on the biased sums. */
#define NVIT_SWIGLU_BWD_TILE_ROWS 256
#define NVIT_SWIGLU_BWD_PART_ROWS 128
/* Tile scheduling of the persistent NT GEMM kernels: 0 = static round-robin (default), 1 = dynamic per-XCD ticket
 * counters: robust when other kernels (RCCL) hold some CUs.  The data-parallel wrapper (parallel.py) selects dynamic. */
int nvit_set_gemm_sched(int dynamic);
/* Kernel selection for tests (-1 = the built-in default).  nt_impl: 0 = 128x128 kernel only,
 * 1 = persistent 256-row kernels for large problems (default), 2 = persistent kernels whatever the tile count;
 * tn_impl: 0 = 128x128 kernel only, 1 = persistent 256x256 kernel for eligible shapes (default). */
int nvit_set_gemm_impl(int nt_impl, int tn_impl);
int nvit_gemm_nt_fusable(int dt, int M, int N, int K);
int nvit_gemm_nt_swiglu_bwd(int dt, const void* A, int lda, const void* B, int ldb, const void* uv, void* duv,
                            float* part, int M, int F, int K, const float* gs, float gscale, void* stream);
int nvit_gemm_nt_swiglu(int dt, const void* A, int lda, const void* B, int ldb, void* uv, void* xm, int M, int F,
                        int K, const float* gs, float gscale, const float* bias, void* stream);
/* nvit_gemm_nt_swiglu_act: nvit_gemm_nt_swiglu for a forward that no backward follows (no_grad / evaluation): the same
 * kernel, operands and gate arithmetic, but only xm[M,F] is written - the raw uv[M,2F], two thirds of the epilogue's
 * stores, is not.  xm is bit-identical to nvit_gemm_nt_swiglu's.  Same eligibility (nvit_gemm_nt_fusable(dt, M, 2F, K)). */
int nvit_gemm_nt_swiglu_act(int dt, const void* A, int lda, const void* B, int ldb, void* xm, int M, int F, int K,
                            const float* gs, float gscale, const float* bias, void* stream);
/* q_prescale: extra factor folded into the q part (qh = q_prescale * sqk*c_q * unit vector, one rounding); pass the same
 * value to nvit_attn_fwd_bounded / nvit_attn_bwd_qknorm.  1 = plain. */
int nvit_gemm_nt_qknorm(int dt, const void* A, int lda, const void* B, int ldb, int M, int K, int nparts, int part0,
                        const float* sqk, float c_q, float q_prescale, void* qh, void* kh, void* vh, float* rq, float* rk,
                        int T, int H, int d, const float* bias, void* stream);

/* nvit_gemm_tn: weight gradient  G[N,K] (+)= sum_m A[m,N-col] * B[m,K-col]  over Mred rows.
 * A [Mred, N] (lda), B [Mred, K] (ldb) of type dt.  Split over `splits` row chunks into the
 * fp32 workspace ws [splits, N, K] (ws_bytes >= splits*N*K*4 + 256; the tail is no longer used - zero padding
 * comes from a device array owned by the library), then reduced in fixed order
 * (deterministic) into G (fp32, ld = ldg): G[perm(n)] = (accumulate ? G : 0) + sum.
 * perm as in nvit_shadow_weights (maps shadow row n to master row). */
int nvit_gemm_tn(int dt, const void* A, int lda, const void* B, int ldb, float* G, int ldg, int Mred, int N,
                 int K, int splits, float* ws, int64_t ws_bytes, int perm, int accumulate, void* stream);

/* ---- row-wise fused ops on the fp32 residual stream --------------------------------
 * nvit_lerp_fwd: out = nrm(nrm(h) + |alpha*c_a| * (nrm(y) - nrm(h)))   (model.py:134-142,159-167)
 * if skip_x != NULL additionally out = nrm(out*skip[0] + skip_x)         (norm_skip, model.py:84-87,452)
 * h, skip_x fp32 [M,C]; y of type y_dt; out fp32; out_lo (type dt, may be NULL) = cast(out).  gate, rows_per_sample: the
 * "gate (optional)" paragraph under nvit_lerp_bwd below.
 * Every row kernel of this section (and nvit_pool_ln_*, nvit_scatter_rows) holds a row of at most NVIT_MAX_EMBD columns.
 * The backward kernels that leave per-workgroup partial sums take nblk <= NVIT_MAX_PART_BLOCKS workgroups; those that
 * leave them per WAVE write NVIT_ROW_WAVES rows per workgroup. */
#define NVIT_MAX_EMBD 2048
#define NVIT_MAX_PART_BLOCKS 4096
#define NVIT_ROW_WAVES 4
#define NVIT_ROW_GRID_MAX 2048 /* the forward row kernels launch at most this many workgroups and stride over the rest */
int nvit_lerp_fwd(int dt, const float* h, const void* y, int y_dt, const float* alpha, float c_a,
                  const float* skip_x, const float* skip, const float* gate, int rows_per_sample, float* out,
                  void* out_lo, int M, int C, void* stream);
/* nvit_lerp_bwd: given dout, recomputes the forward and writes dh (fp32; += if accum_dh), dy (fp32
 * and/or type-dt copy, either may be NULL), dskip_x (fp32, written, only if skip_x), and per-WAVE
 * partial sums part_dlam [NVIT_ROW_WAVES*nblk, C] (d/d|alpha*c_a|) and part_dskip [NVIT_ROW_WAVES*nblk] (if skip_x).
 * nblk = number of workgroups the caller sizes the partial buffers for (<= NVIT_MAX_PART_BLOCKS).
 * dout_add (bf16 [M,C] or NULL): the incoming gradient is dout + dout_add - lets the data-gradient GEMM that produced
 * dout_add store bf16 once instead of read-modify-writing the fp32 dout (the reference's autocast nn.Linear hands its
 * input gradient back in bf16 as well).
 * gate (optional; stochastic depth): NULL = none, and rows_per_sample is ignored.  Otherwise rows m*rows_per_sample ..
 * belong to sample m, M is a multiple of rows_per_sample, and gate[m] (fp32, one per sample: the row of
 * nvit_droppath_draw's table for this block and branch) multiplies the step of the LERP for all of them:
 * out = nrm(nrm(h) + (gate * |alpha*c_a|) * (nrm(y) - nrm(h))); the fused norm_skip is not gated.  The backward is that of
 * the gated forward: dy and the part_dlam terms carry the gate.  With every gate 1.0f the bits are those of gate == NULL.
 * With a gate nvit_lerp_bwd is built for the two calls of the block chain: skip_x without accum_dh (the MLP half) or
 * accum_dh without skip_x (the attention half); any other gated call is an error. */
/* nvit_lerp_bwd_blocks: the nblk that fills the device exactly once for the kernel variant these options select (0 on
 * error, and for a gated variant that is not built); callers size the partial buffers with it. */
int nvit_lerp_bwd_blocks(int dt, int y_dt, int C, int has_add, int has_skip, int accum, int gated);
int nvit_lerp_bwd(int dt, const float* dout, const void* dout_add, const float* h, const void* y, int y_dt, const float* alpha,
                  float c_a, const float* skip_x, const float* skip, const float* gate, int rows_per_sample, float* dh,
                  int accum_dh, float* dy, void* dy_lo, float* dskip_x, float* part_dlam, float* part_dskip, int nblk,
                  int M, int C, void* stream);

/* RMSNorm (model.py:170-182; not on the nViT path, provided so that the public module works):
 * out = x * rsqrt(mean(x^2) + eps) * w, fp32 [M, C]; rstd [M] saved for the backward.
 * nvit_rmsnorm_bwd: dx [M, C] and part_dw [nblk, C] (per-workgroup partial sums of d(w); reduce with nvit_colsum_reduce). */
int nvit_rmsnorm_fwd(const float* x, const float* w, float eps, float* out, float* rstd, int M, int C, void* stream);
int nvit_rmsnorm_bwd(const float* dout, const float* x, const float* w, const float* rstd, float* dx, float* part_dw,
                     int nblk, int M, int C, void* stream);
/* Residual + RMSNorm row kernels of the plain-ViT block (use_nvit=False, model.py:92-169 with the RMSNorm modules built):
 * nvit_res_rmsnorm_fwd: out = z * rsqrt(mean(z^2) + eps) * w, z = a + y (y of type y_dt, or NULL: z = a); out fp32
 * [M,C], out_lo (type dt, may be NULL) = cast(out), rstd [M].  z itself is not stored.
 * nvit_res_rmsnorm_bwd: from g (+ g_add, type dt, may be NULL: a data-gradient GEMM's output) recomputes z = a + y and
 * writes dz fp32 (added to dz if accum), dz_lo (type dt, may be NULL) = cast(dz), and per-WAVE partial sums part_dw
 * [NVIT_ROW_WAVES*nblk, C] of d(w) (reduce with nvit_colsum_reduce).  nblk <= NVIT_MAX_PART_BLOCKS workgroups.
 * nvit_res_skip_fwd: out = nrm((h + y) * skip[0] + x)  (norm_skip after a plain-ViT block, model.py:84-87,450-452);
 * h, x fp32 [M,C], y of type y_dt; out fp32, out_lo (type dt, may be NULL) = cast(out).
 * nvit_res_skip_bwd: dx = d(x) fp32 (written), dh = d(h + y) fp32, dh_lo (type dt, may be NULL) = cast(dh), and per-WAVE
 * partial sums part_dskip [NVIT_ROW_WAVES*nblk] of d(skip).
 * gate (optional; stochastic depth of the plain-ViT block chain): NULL = none, and rows_per_sample is ignored.  Otherwise
 * gate is fp32, one per sample, rows m*rows_per_sample .. belong to sample m, M is a multiple of rows_per_sample, and the
 * branch output enters as gate * y wherever the kernel adds y: z = a + gate * y (res_rmsnorm, which then requires y),
 * (h + gate * y) (res_skip).  Backward: the fp32 outputs dz / dh stay the gradient of the sum, which goes on down the
 * stream; the type-dt copies dz_lo / dh_lo are gate * that = d(y), what the branch's GEMMs read (fp32 mode included:
 * there the caller can no longer alias the two).  With a gate nvit_res_rmsnorm_bwd is built with the addend g_add only.
 * With every gate 1.0f the bits are those of gate == NULL. */
int nvit_res_rmsnorm_fwd(int dt, const float* a, const void* y, int y_dt, const float* w, float eps, const float* gate,
                         int rows_per_sample, float* out, void* out_lo, float* rstd, int M, int C, void* stream);
int nvit_res_rmsnorm_bwd(int dt, const float* g, const void* g_add, const float* a, const void* y, int y_dt,
                         const float* w, const float* rstd, const float* gate, int rows_per_sample, float* dz, int accum,
                         void* dz_lo, float* part_dw, int nblk, int M, int C, void* stream);
int nvit_res_skip_fwd(int dt, const float* h, const void* y, int y_dt, const float* skip, const float* x,
                      const float* gate, int rows_per_sample, float* out, void* out_lo, int M, int C, void* stream);
int nvit_res_skip_bwd(int dt, const float* dout, const float* h, const void* y, int y_dt, const float* skip,
                      const float* x, const float* gate, int rows_per_sample, float* dh, void* dh_lo, float* dx,
                      float* part_dskip, int nblk, int M, int C, void* stream);
/* Block.norm_skip on its own (model.py:84-87): out = nrm(src*skip[0] + tgt), fp32 [M,C]; backward writes dsrc, dtgt
 * (tgt == NULL / dtgt == NULL: the target term is absent, i.e. justnorm(src*skip[0]), model.py:43-44,89-90)
 * and part_dskip [nblk]. (ViT.forward uses the copy fused into nvit_lerp_fwd/bwd.) */
int nvit_norm_skip_fwd(const float* src, const float* tgt, const float* skip, float* out, int M, int C, void* stream);
int nvit_norm_skip_bwd(const float* dout, const float* src, const float* tgt, const float* skip, float* dsrc,
                       float* dtgt, float* part_dskip, int nblk, int M, int C, void* stream);

/* nvit_qknorm_fwd: per-head cosine normalise + learned scale + head split (model.py:104-119,231-247)
 * q/k/v sources: row-major, type dt, row stride ld* elements, C columns each.
 * qh = (sqk*c_q) * nrm_d(q) etc. written [B,H,T,d] type dt; v copied to [B,H,T,d];
 * rq, rk [M,H] fp32 = 1/||q_head||.
 * sqk == NULL: the head split alone (plain-ViT attention, model.py:97-100): q, k, v copied to [B,H,T,d] as they are
 * (type conversion only); rq, rk are not written.
 * d in {16, 32, 64, 128}, H*d <= NVIT_MAX_EMBD.  nvit_qknorm_bwd and nvit_heads_pad_bwd below run one kernel
 * (heads_merge_kernel, templated on the stored head width: here d itself); the forward has a kernel per layout. */
int nvit_qknorm_fwd(int dt, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv,
                    const float* sqk, float c_q, void* qh, void* kh, void* vh, float* rq, float* rk, int B,
                    int T, int H, int d, void* stream);
/* nvit_qknorm_bwd: dq/dk/dv (type dt, row strides ld*) from dqh/dkh/dvh [B,H,T,d]; part_dsqk
 * [nblk, C] partial sums of d/d(sqk*c_q).
 * sqk == NULL: the backward of the plain split, i.e. the head merge dq/dk/dv = dqh/dkh/dvh (dt F32 or BF16; qh, kh, rq, rk,
 * part_dsqk and nblk are not used). */
int nvit_qknorm_bwd(int dt, const void* dqh, const void* dkh, const void* dvh, const void* qh, const void* kh,
                    const float* rq, const float* rk, const float* sqk, float c_q, void* dq, int ldq,
                    void* dk, int ldk, void* dv, int ldv, float* part_dsqk, int nblk, int B, int T, int H,
                    int d, void* stream);

/* ---- zero-padded heads: head dims d that are no power of two on the dp = NVIT_PAD_HEAD_DIM attention kernels ----
 * The head tensors are [B,H,T,dp] with columns d..dp-1 stored as zeros (no score, no output column < d and no gradient
 * column < d changes); nvit_attn_fwd / _fwd_bounded / _bwd then run at head dim dp with the scale of the REAL d.
 * dp = NVIT_PAD_HEAD_DIM, d % 8 == 0, 0 < d < dp, H*d <= NVIT_MAX_EMBD, any B*T >= 1.  Deterministic, no atomics.
 * The backward kernel is that of nvit_qknorm_bwd at stored head width dp; lanes on a pad column load nothing.
 * nvit_heads_pad_fwd: nvit_qknorm_fwd from fp32 projections (dt NVIT_F32: fp32 head tensors, NVIT_BF16_F32IN: bf16)
 *   into qh, kh, vh [B,H,T,dp]; EVERY pad column is stored (as +0) on every launch.  sqk (compact [H*d]) given: the sum
 *   of squares over the d real columns from the unrounded projections, rq, rk [M,H], and - sqk_pad not NULL - sqk_pad
 *   [H*dp] = sqk with zero pads (what nvit_attn_fwd_bounded indexes at head dim dp).  sqk NULL: the split alone.
 * nvit_heads_pad_bwd: nvit_qknorm_bwd (same formulas; sqk NULL: the merge alone) reading the first d columns of
 *   dqh, dkh, dvh, qh, kh [B,H,T,dp] (type dt); dq/dk/dv token-major (type dt, row strides ld*), part_dsqk [nblk, H*d]
 *   in compact channel order.
 * nvit_pad_cols:   dst [M, H*dp] = src [M, H*d] with zero pads (dO; O for the dQ kernel's rowsum(dO*O) over dp columns).
 * nvit_unpad_cols: dst [M, H*d] = the first d columns of every head of src [M, H*dp] (O for the output projection). */
#define NVIT_PAD_HEAD_DIM 128
int nvit_heads_pad_fwd(int dt, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                       const float* sqk, float c_q, void* qh, void* kh, void* vh, float* rq, float* rk,
                       float* sqk_pad, int B, int T, int H, int d, int dp, void* stream);
int nvit_heads_pad_bwd(int dt, const void* dqh, const void* dkh, const void* dvh, const void* qh, const void* kh,
                       const float* rq, const float* rk, const float* sqk, float c_q, void* dq, int ldq,
                       void* dk, int ldk, void* dv, int ldv, float* part_dsqk, int nblk, int B, int T, int H,
                       int d, int dp, void* stream);
int nvit_pad_cols(int dt, const void* src, void* dst, int M, int H, int d, int dp, void* stream);
int nvit_unpad_cols(int dt, const void* src, void* dst, int M, int H, int d, int dp, void* stream);

/* nvit_swiglu_fwd: x[m,j] = (gu*u) * silu(gv*v), u = uv[m, 32*(j/16) + j%16], v = uv[m, 32*(j/16)+16+j%16]
 * (interleaved GEMM output, see perm=1), gu = gscale*suv[j], gv = gscale*suv[F+j]; suv may be NULL (=1)
 * (model.py:148-154 with gscale = sqrt(C); cross-attention gate model.py:259-261 with suv=NULL). */
int nvit_swiglu_fwd(int dt, const void* uv, const float* suv, float gscale, void* x, int M, int F, void* stream);
/* nvit_swiglu_bwd: duv (interleaved, type dt) and part_dsuv [nblk_rows, 2F] (natural order, d/d(suv),
 * already multiplied by gscale; skipped if suv NULL). rows_per_blk rows per partial. */
int nvit_swiglu_bwd(int dt, const void* dx, const void* uv, const float* suv, float gscale, void* duv,
                    float* part_dsuv, int rows_per_blk, int M, int F, void* stream);

/* nvit_colsum_reduce: out[n] (+)= f(sum_b part[b, n]).  kind 0: plain*scale; kind 1: sum * sign(ref[n]*scale) * scale
 * (d|alpha c_a| -> d alpha); kind 2: plain*scale written to out[perm1(n)] (SwiGLU interleave -> natural order). */
int nvit_colsum_reduce(const float* part, int nblk, int N, float* out, int accumulate, int kind, const float* ref,
                       float scale, void* stream);
/* nvit_colsum_reduce_multi: up to NVIT_COLSUM_REDUCE_MAX_ITEMS such reductions in ONE launch (host arrays of n entries;
 * pointers as int64).  An item may name a second partial array part_b (0 = none) whose reduced, scaled sum is added after
 * the first one's. */
#define NVIT_COLSUM_REDUCE_MAX_ITEMS 8
int nvit_colsum_reduce_multi(const int64_t* part, const int* nblk, const int64_t* part_b, const int* nblk_b, const int* N,
                             const int64_t* out, const int* accumulate, const int* kind, const int64_t* ref,
                             const float* scale, int n, void* stream);
/* nvit_colsum: out[n] (+)= scale * sum_r a[r,n] * (b ? b[r,n] : 1) over R rows; a,b fp32 or dt (a_dt,b_dt);
 * `period`>0 folds rows modulo period: out[(r%period), n] (pos-embed gradients). */
int nvit_colsum(const void* a, int a_dt, int lda, const void* b, int b_dt, int ldb, int R, int N, int period,
                float* out, int accumulate, float scale, void* stream);
int nvit_cast(const float* src, void* dst, int dt, int64_t n, void* stream);
/* Input pipeline, deterministic part (train.py:1084-1090): ToTensor + kornia Normalize(mean, std) in one pass.
 * in: uint8 [B,H,W,C] (in_is_u8_hwc = 1; scaled by 1/255 first) or fp32 [B,C,H,W] already in [0,1]; out fp32 [B,C,H,W]
 * = (in - mean) / std.  (The randomised half of that pipeline: nvit_augment_draw / nvit_augment_apply below.) */
int nvit_normalize_images(const void* in, int in_is_u8_hwc, float* out, int B, int C, int H, int W, float mean, float std_,
                          void* stream);
/* On-device AutoAugment: the randomised half of the input pipeline, two launches per batch, no host
 * synchronisation, capturable in a hipGraph.  The ops are Pillow's, bit for bit (tests/augment_ref.py).
 * nvit_augment_draw: params int32 [B,2,NVIT_AUG_ROW] = per image two ops, each (op id, seven arguments).  One
 * Philox4x32-10 call per image, key = seed, counter = (first_index + i, *step): r0 picks one of the P sub-policies, r1/r2
 * gate its two ops against their probabilities (an op left out becomes Identity), bits 0/1 of r3 are their signs.
 * policy: device int32 [P,2,3] = (op id, probability as fp32 bits, magnitude index below NVIT_AUG_NMAG); argtab: device
 * int32 [NVIT_AUG_NOPS,NVIT_AUG_NMAG,2,NVIT_AUG_ROW], the parameter row of every (op, magnitude index, sign) at this
 * image size (the host computes it in fp64).  *step is a device int64 that the kernel reads and then advances by one, so
 * a graph replay draws fresh parameters.  Image sides of nvit_augment_apply / nvit_mix_* are at most NVIT_AUG_MAX_SIDE
 * (16.16 coordinates in 32 bits). */
#define NVIT_AUG_ROW 8
#define NVIT_AUG_NOPS 15
#define NVIT_AUG_NMAG 10
#define NVIT_AUG_MAX_SIDE 4096
int nvit_augment_draw(const int* policy, int P, uint64_t seed, int64_t* step, int64_t first_index, const int* argtab,
                      int* params, int B, void* stream);
/* nvit_augment_apply: in uint8 [B,H,W,C], C in {1,3}; per image the two ops of params in sequence, the second on the
 * complete result of the first.  out_f32 (may be NULL): fp32 [B,C,H,W] = (x/255 - mean) / std with the arithmetic of
 * nvit_normalize_images (needs W % 4 == 0); out_u8 (may be NULL): the augmented uint8 [B,H,W,C].  ws: caller-provided
 * workspace of ws_bytes >= 2 * B * round_up(H*W*C, 256) bytes. */
int nvit_augment_apply(const void* in, const int* params, float* out_f32, void* out_u8, void* ws, int64_t ws_bytes, int B,
                       int H, int W, int C, float mean, float std_, void* stream);
/* On-device RandAugment (tests/randaug_ref.py): timm's rand-m9-mstd0.5-inc1 family in AutoAugment's place.
 * Parameter table int32 [B,num_layers,NVIT_RA_ROW], per row: [0] op id (0 = layer off; 1..14 AutoAugment's ids,
 * NVIT_RA_SOLARIZE_ADD the one new op), [1] filter of a geometric op (NVIT_RA_BILINEAR / NVIT_RA_BICUBIC), then for the
 * geometric ops (ids 1..5) six fp64 output-to-input coefficients a0..a5 in ints 2..13 (8-byte aligned), for every other
 * op its argument in int 2 (fp32 bits of an enhancement factor, bits kept, threshold, or the amount added); the rest 0.
 * nvit_randaug_draw: one Philox4x32-10 call per (image, layer), counter = (first_index + b, *step), key = seed with (a
 * domain constant + layer) xor-ed into its high word: (r0 * NVIT_RA_NCHOICES) >> 32 picks the op in timm's list order,
 * (r1 >> 8) * 2^-24 < prob switches it on, r2 >> 8 is the magnitude's 24-bit uniform, bit 0 of r3 the sign (1 negates),
 * bit 1 of r3 the filter when interp == NVIT_RA_RANDOM.  Magnitude m: `magnitude` (mstd == 0), magnitude * u (mstd
 * infinite), else magnitude + mstd * z with z interpolated from q, device fp64 [NVIT_ERASE_KNOTS + 1] normal quantiles;
 * then clamped to [0, mmax].  The level maps are timm's, in fp64.  Rotate's cos / sin come from rot, device fp64
 * [2, NVIT_RA_ROT_KNOTS + 1] (cos, then sin) over [0, 3 * mmax] degrees, linearly between knots: no transcendental runs
 * on the device.  *step is a device int64 that the kernel reads and then advances by one, as nvit_augment_draw does. */
#define NVIT_RA_ROW 16
#define NVIT_RA_NCHOICES 15
#define NVIT_RA_SOLARIZE_ADD 15
#define NVIT_RA_NOPS 16 /* op ids known to nvit_randaug_apply: 0..15 */
#define NVIT_RA_MAX_LAYERS 4
#define NVIT_RA_ROT_KNOTS 1024
#define NVIT_RA_BILINEAR 0
#define NVIT_RA_BICUBIC 1
#define NVIT_RA_RANDOM 2
int nvit_randaug_draw(uint64_t seed, int64_t* step, int64_t first_index, const double* q, const double* rot, double magnitude,
                      double mstd, double mmax, int increasing, float prob, int interp, double translate_pct, int* params,
                      int B, int num_layers, int H, int W, void* stream);
/* nvit_randaug_apply: in uint8 [B,H,W,C], C in {1,3}; per image the num_layers ops of params in sequence, each on the
 * complete result of the one before.  Geometric ops are Pillow's ImagingGenericTransform in fp64 with the BILINEAR or
 * BICUBIC filter; a pixel whose source lies outside the image takes fill0..fill2 (one value per channel).  The other ops
 * are nvit_augment_apply's.  Outputs and workspace as for nvit_augment_apply. */
int nvit_randaug_apply(const void* in, const int* params, float* out_f32, void* out_u8, void* ws, int64_t ws_bytes, int B,
                       int H, int W, int C, int num_layers, int fill0, int fill1, int fill2, float mean, float std_,
                       void* stream);
/* On-device Mixup / CutMix (tests/mix_ref.py): rows p and B-1-p of the batch form pair p (the middle row of
 * an odd batch is its own partner and stays unmixed).
 * nvit_mix_draw: one Philox4x32-10 call per pair, key = seed with a domain constant xor-ed into its high word, counter =
 * (first_index + p, *step): r0 gates the pair against prob, r1 picks CutMix against switch_prob (only when both modes are
 * on), r2 indexes the mode's quantile table (q_mix / q_cut: device fp32 [NVIT_MIX_KNOTS + 1], the Beta(alpha,alpha) quantile
 * at k/NVIT_MIX_KNOTS, computed by the host in fp64; NULL switches the mode off) and interpolates lambda linearly, r3 is
 * the box centre.  The CutMix box and its corrected lambda (timm's rand_bbox, correct_lam) are computed in fp64.
 * Written: table int32 [B,NVIT_MIX_ROW] =
 * (mode 0 none / 1 Mixup / 2 CutMix, lambda as fp32 bits, y0, y1, x0, x1, partner row, 0), lam fp32 [B] and
 * y2 int64 [B] = labels[partner]; both rows of a pair carry the same lambda and box.  *step is a device int64 that the
 * kernel reads and then advances by one, as nvit_augment_draw does. */
#define NVIT_MIX_ROW 8
#define NVIT_MIX_KNOTS 1024
int nvit_mix_draw(uint64_t seed, int64_t* step, int64_t first_index, const float* q_mix, const float* q_cut, float prob,
                  float switch_prob, const int64_t* labels, int* table, float* lam, int64_t* y2, int B, int H, int W,
                  void* stream);
/* nvit_mix_apply: in, out fp32 [B,C,H,W], W % 4 == 0; out may be in (in place).  Mixup: out_i = lam * x_i + (1 - lam) * x_j
 * (two rounded products, one add); CutMix: rows i and j exchange the pixels of [y0,y1) x [x0,x1) in every channel.  A row
 * of mode 0, a row that is its own partner, and a row whose partner does not name it back with the same mode is copied. */
int nvit_mix_apply(const float* in, const int* table, float* out, int B, int C, int H, int W, void* stream);
/* Stochastic depth (DropPath; tests/droppath_ref.py).  nvit_droppath_draw: table fp32 [2*n_layer, B], row
 * 2*l + br = the gates of branch br (0 attention, 1 MLP) of block l, one per sample: 0.0f (dropped) or, kept, 1.0f /
 * keep_l (scale_by_keep != 0) or 1.0f, keep_l = 1.0f - rates[l] (rates: device fp32 [n_layer], each in [0, 1)).  One
 * Philox4x32-10 call per gate, counter = (first_index + b, *step), key = seed with (a domain constant + the row index)
 * xor-ed into its high word; the sample is kept iff (r0 >> 8) * 2^-24 < keep_l.  At most NVIT_DROPPATH_MAX_GATES gates per
 * call.  *step is a device int64 that the kernel reads and then advances by one, as nvit_augment_draw does. */
#define NVIT_DROPPATH_MAX_GATES 1048576
int nvit_droppath_draw(uint64_t seed, int64_t* step, int64_t first_index, const float* rates, int scale_by_keep,
                       float* table, int n_layer, int B, void* stream);
/* Patch dropout (timm's PatchDropout / FLIP; tests/patchdrop_ref.py).  nvit_patchdrop_draw: keep int32 [B,K],
 * the kept token indices of each sample, ascending; slot int32 [B,T], slot[b, keep[b,j]] = j and -1 for a dropped token.
 * Token t of sample b gets the 24-bit word u = r >> 8, r = word t & 3 of one Philox4x32-10 call, counter = (first_index +
 * b, *step), key = seed with (a domain constant + (t >> 2)) xor-ed into its high word; kept are the K tokens with the
 * smallest (u << 32) | t, so a tie of u goes to the smaller t.  One workgroup per sample, 1 <= K <= T <=
 * NVIT_PATCHDROP_MAX_TOKENS.  *step is a device int64 that every workgroup reads; a one-thread launch that the call puts
 * behind the draw on the same stream advances it by one (nvit_augment_draw's contract, for a grid of more than one
 * workgroup). */
#define NVIT_PATCHDROP_MAX_TOKENS 4096
int nvit_patchdrop_draw(uint64_t seed, int64_t* step, int64_t first_index, int* keep, int* slot, int B, int T, int K,
                        void* stream);
/* nvit_rows_gather: dstX[b*K + j, :] = srcX[b*T + keep[b,j], :], fp32 rows of C contiguous elements (C a multiple of 4,
 * 16-byte aligned pointers), X = 0 and, src1 / dst1 non-NULL, 1: both embedding streams in one launch.  loX non-NULL
 * (lo_dt NVIT_BF16; lo1 exactly when lo0 and src1): the row is also stored rounded to bf16, round to nearest even as
 * nvit_cast does.  A keep entry outside [0, T) stores a row of zeros.  nvit_rows_scatter is its backward: gX[b*T + t, :] =
 * dX[b*K + slot[b,t], :] where 0 <= slot[b,t] < K, else zeros; every element of gX is written exactly once (no memset,
 * no atomics).  Grids as the forward row kernels': NVIT_ROW_WAVES rows per workgroup, at most NVIT_ROW_GRID_MAX. */
int nvit_rows_gather(const float* src0, const float* src1, const int* keep, float* dst0, float* dst1, void* lo0, void* lo1,
                     int lo_dt, int B, int T, int K, int C, void* stream);
int nvit_rows_scatter(const float* d0, const float* d1, const int* slot, float* g0, float* g1, int B, int T, int K, int C,
                      void* stream);
/* The device-resident dataset ("The device-resident dataset"; tests/loader_ref.py).  nvit_loader_draw: idx
 * int64 [B], the images of rows [first_row, first_row + B) of the global batch at step s = *step.  With S =
 * steps_per_epoch and G = global_batch: epoch = s / S, row i sits at position q = (s % S) * G + first_row + i and shows
 * image perm(q / repeats), or q / repeats itself with shuffle == 0; S * G <= N * repeats, so q / repeats < N.  perm is a
 * bijection of [0, N) per (seed, epoch): a 4-round balanced Feistel network on w bits, w the smallest even number of bits
 * that holds N - 1 (at least 2), round j mapping (L, R) to (R, L ^ (v[0] & mask)) with v = Philox4x32-10 of counter (R,
 * j, epoch low, epoch high) and key = seed with a domain constant xor-ed into its high word; the network is re-applied
 * while the value is >= N.  record int64 [NVIT_LOADER_RECORD] receives {epoch, s % S}.  One workgroup: every thread reads
 * *step, then, behind a barrier, one thread stores s + 1 (no tick launch).
 * nvit_loader_gather: out[b, :] = images[idx[b], :], rows of row_bytes bytes, and y[b] = labels[idx[b]]; offsets are 64
 * bits wide.  16-byte loads and stores when row_bytes % 16 == 0 and both bases are 16-byte aligned, bytes otherwise.  An
 * index outside [0, N) reads nothing: the row becomes zeros and the label 0. */
#define NVIT_LOADER_MAX_IMAGES 1099511627776 /* 2^40 */
#define NVIT_LOADER_MAX_BATCH 65536
#define NVIT_LOADER_MAX_REPEATS 1024
#define NVIT_LOADER_RECORD 2
int nvit_loader_draw(uint64_t seed, int64_t* step, int64_t N, int64_t steps_per_epoch, int64_t global_batch,
                     int64_t first_row, int repeats, int shuffle, int64_t* idx, int64_t* record, int B, void* stream);
int nvit_loader_gather(const void* images, const int64_t* labels, const int64_t* idx, void* out, int64_t* y, int64_t N,
                       int64_t row_bytes, int B, void* stream);
/* Resampling a position-embedding table to another token grid (timm's resample_abs_pos_embed; DESIGN.md §4;
 * nvit_amd/resample.py builds the tables).  nvit_pos_resample_fwd: pX fp32 [g*g, C] -> outX fp32 [g2*g2, C], the bicubic
 * (a = -0.5), antialiased, align_corners = false resize of the g x g grid of C-vectors: out[oy*g2 + ox, :] = sum over ty, tx
 * of (wy[ty] * wx[tx]) * p[(y0 + ty)*g + x0 + tx, :], taps in this order, one product rounding for the weight and one fused
 * multiply-add per tap.  taps: device int32 [g2, 2 + NVIT_POS_RESAMPLE_MAX_TAPS], row o = (first source index, tap count,
 * the weights as fp32 bit patterns), computed by the host in fp64; the same row serves as y row and as x row.  X = 0 and,
 * p1 / out1 non-NULL, 1: both tables of the model in one launch.  nvit_pos_resample_bwd is the exact adjoint, dX fp32
 * [g2*g2, C] -> gX fp32 [g*g, C], the same gather driven by the transposed table taps_t int32 [g, 2 + MAX_TAPS] (row i = the
 * outputs that read source i and their weights): every element of gX is written exactly once, no atomics, fixed order.
 * C a multiple of 4, at most NVIT_MAX_EMBD; 16-byte aligned pointers; g != g2 (equal grids are the caller's no-op), both at
 * most NVIT_POS_RESAMPLE_MAX_GRID.  A table entry that points outside the source grid is clipped to it, not followed. */
#define NVIT_POS_RESAMPLE_MAX_TAPS 32
#define NVIT_POS_RESAMPLE_MAX_GRID 1024
int nvit_pos_resample_fwd(const float* p0, const float* p1, const int* taps, float* out0, float* out1, int g, int g2, int C,
                          void* stream);
int nvit_pos_resample_bwd(const float* d0, const float* d1, const int* taps_t, float* g0, float* g1, int g, int g2, int C,
                          void* stream);
/* On-device RandomResizedCrop + horizontal flip (tests/crop_ref.py): a stored uint8 [B,Hs,Ws,C] batch ->
 * uint8 [B,size,size,C], image b = Pillow's crop(box b).resize((size, size), BILINEAR | BICUBIC), mirrored if its flip
 * bit is set, bit for bit.  Three launches per batch: the draw and the two passes of the apply.
 * nvit_crop_draw: table int32 [B,NVIT_CROP_ROW] = (top, left, h, w, flip, 0, 0, 0), torchvision's get_params in fp64.
 * Philox4x32-10, counter = (first_index + b, *step), key = seed with a domain constant + a xor-ed into its high word:
 * a = 0..NVIT_CROP_ATTEMPTS-1 are the attempts (r0: area in [scale0, scale1], r1: aspect, r2: top, r3: left), a =
 * NVIT_CROP_ATTEMPTS the flip bit (r0 against hflip).  aspect: device fp64 [NVIT_CROP_KNOTS + 1], exp(log ratio_min +
 * k / NVIT_CROP_KNOTS * (log ratio_max - log ratio_min)), computed by the host and interpolated linearly: no
 * transcendental runs on the device.  After the last failed attempt the box is torchvision's central fallback.  *step
 * is a device int64 that the kernel reads and then advances by one, as nvit_augment_draw does. */
#define NVIT_CROP_ROW 8
#define NVIT_CROP_KNOTS 1024
#define NVIT_CROP_ATTEMPTS 10
#define NVIT_CROP_MAX_SRC 2048
#define NVIT_CROP_MAX_BATCH 65535 /* images per call of nvit_crop_apply / nvit_erase_apply: the grids' second dimension */
#define NVIT_CROP_BILINEAR 0
#define NVIT_CROP_BICUBIC 1
int nvit_crop_draw(uint64_t seed, int64_t* step, int64_t first_index, const double* aspect, double scale0, double scale1,
                   double ratio_min, double ratio_max, float hflip, int* table, int B, int Hs, int Ws, void* stream);
/* nvit_crop_apply: in uint8 [B,Hs,Ws,C], C in {1,3}, sides up to NVIT_CROP_MAX_SRC; out uint8 [B,size,size,C], size % 4
 * == 0, size <= NVIT_AUG_MAX_SIDE.  Pillow's ImagingResample for 8-bit data on the box of table[b]: per axis the integer
 * taps (22 fractional bits) are computed in fp64 by the workgroup that uses them, the horizontal pass writes a uint8
 * [h,size,C] intermediate, the vertical pass reads it and folds the flip into its store index.  A table row whose box
 * leaves the image counts as the whole image.  Taps and intermediate live in ws, ws_bytes >= nvit_crop_ws_bytes(...)
 * (sized for the largest box, the whole image); every byte of out is written. */
int64_t nvit_crop_ws_bytes(int B, int Hs, int Ws, int C, int size, int interp);
int nvit_crop_apply(const void* in, const int* table, void* out, void* ws, int64_t ws_bytes, int B, int Hs, int Ws, int C,
                    int size, int interp, void* stream);
/* On-device Resize + CenterCrop for evaluation batches (tests/center_crop_ref.py): in uint8 [B,Hs,Ws,C], C in
 * {1,3}, one source size per batch, sides up to NVIT_CROP_MAX_SRC.  Image b is Pillow's resize((W2, H2), BILINEAR |
 * BICUBIC).crop((left, top, left + size, top + size)), bit for bit, of which only the window is computed: two launches,
 * the horizontal pass over the window's columns of the source rows that the window's vertical taps read (uint8
 * intermediate), the vertical pass over the window's rows.  H2, W2, top, left, size are host integers: size % 4 == 0 in
 * 4..NVIT_AUG_MAX_SIDE, size <= H2, W2 <= NVIT_AUG_MAX_SIDE, 0 <= top <= H2 - size, 0 <= left <= W2 - size, B up to
 * NVIT_CROP_MAX_BATCH; anything else is refused, nothing is clamped.  There is no table, no draw and no device state.
 * Outputs, either may be NULL but not both, both written by the vertical pass: out_u8 uint8 [B,size,size,C] (4-byte
 * aligned) and out_f32 fp32 [B,C,size,size] (16-byte aligned) = (x / 255 - mean) / std with the roundings of
 * nvit_normalize_images (std > 0).  ws (16-byte aligned) holds the tap sets and the intermediate, ws_bytes >=
 * nvit_center_crop_ws_bytes(...), which is -1 for a refused shape and is sized by the rows read, not by Hs. */
int64_t nvit_center_crop_ws_bytes(int B, int Hs, int Ws, int C, int H2, int W2, int top, int left, int size, int interp);
int nvit_center_crop_apply(const void* in, void* out_u8, float* out_f32, void* ws, int64_t ws_bytes, int B, int Hs, int Ws,
                           int C, int H2, int W2, int top, int left, int size, int interp, float mean, float std,
                           void* stream);
/* On-device RandomErasing (timm's, count 1, per image; tests/crop_ref.py) on the fp32 [B,C,H,W] model input.
 * nvit_erase_draw: table int32 [B,NVIT_ERASE_ROW] = (on, top, left, h, w, noise key low, noise key high, 0).  Philox as in
 * nvit_crop_draw under the erasing's own domain: a = NVIT_CROP_ATTEMPTS is the gate (r0 against prob), a = 0.. the attempts
 * (area in [area0, area1] of H*W, aspect from the same kind of table, accepted if w < W and h < H; no fallback: after the
 * last failed attempt nothing is erased), a = NVIT_CROP_ATTEMPTS + 1 the image's noise sub-key (r0, r1).  As in timm, an
 * attempt whose h or w rounds to 0 (a tiny image or area) is accepted: the row then reads on = 1 with an empty box, whose
 * top / left may equal H / W, and nvit_erase_apply erases nothing for it. */
#define NVIT_ERASE_ROW 8
#define NVIT_ERASE_KNOTS 1024
#define NVIT_ERASE_CONST 0
#define NVIT_ERASE_PIXEL 1
int nvit_erase_draw(uint64_t seed, int64_t* step, int64_t first_index, const double* aspect, double area0, double area1,
                    float prob, int* table, int B, int H, int W, void* stream);
/* nvit_erase_apply: in, out fp32 [B,C,H,W], W % 4 == 0; out may be in (in place).  The box of table[b] is overwritten in
 * every channel, by 0.0 (NVIT_ERASE_CONST) or by N(0,1) noise (NVIT_ERASE_PIXEL): float4 number e of the image takes
 * Philox(counter = (e,0,0,0), key = the image's sub-key), and each of the four words indexes q, device fp32
 * [NVIT_ERASE_KNOTS + 1] = the normal quantile at k / NVIT_ERASE_KNOTS with finite end knots, linearly between knots.
 * Everything else is copied (left alone in place).  A row whose box leaves the image erases nothing. */
int nvit_erase_apply(const float* in, const int* table, const float* q, float* out, int mode, int B, int C, int H, int W,
                     void* stream);
/* out[r,n] = a[r,n] * s[n] * c   (sz scaling model.py:466-468 and its backward); s == NULL: out = a * c */
int nvit_scale_cols(const float* a, int lda, const float* s, float c, void* out, int out_dt, int ldo, int R, int N,
                    void* stream);

/* ---- attention ------------------------------------------------------------------------
 * O = softmax(scale * qh kh^T) vh per (b,h), non-causal, no mask (model.py:121-124 SDPA branch).
 * qh,kh,vh [B,H,T,d] type dt; o [B,T,H*d] type dt (heads merged, model.py:127); lse [B,H,T] fp32
 * (natural log of the softmax denominator, including the running max).  d in {32,64,128}.
 * impl: 0 = scalar-FMA reference kernel (any dt), 1 = MFMA flash kernel (bf16 only); both take every d above. */
int nvit_attn_fwd(int dt, int impl, const void* qh, const void* kh, const void* vh, float scale, void* o, float* lse,
                  int B, int H, int Tq, int Tk, int d, void* stream);
/* Same, for the nViT call sites where q and k are (sqk*c_q) * unit vectors per head (model.py:108-112): every score is
 * bounded by max_d (sqk_d*c_q)^2, and while that bound is small (it is 1 at initialisation) the MFMA kernel takes
 * probabilities relative to the bound instead of a running maximum (no per-tile max / rescale).  sqk: [H*d] fp32;
 * NULL: no bound - the running-maximum kernel on a q pre-scaled by q_prescale (plain-ViT heads from the split-only
 * nvit_gemm_nt_qknorm).
 * q_prescale > 0: qh holds q_prescale * q_hat (see nvit_gemm_nt_qknorm); the result is that of the un-scaled q.  With
 * q_prescale = scale * log2(e) the exponent of the MFMA kernel needs no multiply: the score accumulator starts at minus
 * the bound and goes straight into v_exp_f32 (one VALU instruction less per score in a VALU-bound kernel).
 * d in {32,64,128}, as nvit_attn_fwd. */
int nvit_attn_fwd_bounded(int dt, int impl, const void* qh, const void* kh, const void* vh, float scale, const float* sqk,
                          float c_q, float q_prescale, void* o, float* lse, int B, int H, int Tq, int Tk, int d,
                          void* stream);
/* delta: [2,B,H,Tq] fp32 workspace (MINUS rowsum(dO*O) and MINUS lse in log2 units - accumulator seeds of the dk/dv
 * kernel). dqh,dkh,dvh [B,H,T,d] type dt.  d in {32,64,128}, impl as nvit_attn_fwd. */
int nvit_attn_bwd(int dt, int impl, const void* dout, const void* qh, const void* kh, const void* vh, const void* o,
                  const float* lse, float scale, void* dqh, void* dkh, void* dvh, float* delta, int B, int H,
                  int Tq, int Tk, int d, void* stream);

/* nvit_attn_bwd_qknorm: MFMA attention backward (bf16, d=64) with nvit_qknorm_bwd fused into the epilogues:
 * writes token-major dq/dk/dv (type bf16, row stride ld elements, head h at column h*64) and the partial sums
 * part_q [B*ceil(Tq/NVIT_ATTN_BWD_PART_ROWS), C], part_k [B*ceil(Tk/NVIT_ATTN_BWD_PART_ROWS), C] of d/d(sqk*c_q) (reduce
 * with nvit_colsum_reduce).
 * q_prescale: the factor the producer folded into qh (see nvit_attn_fwd_bounded); gradients are those of the plain form.
 * sqk == NULL (plain-ViT heads): dq/dk/dv stored token-major as they are; rq, rk, c_q, part_q, part_k are not used. */
#define NVIT_ATTN_BWD_PART_ROWS 128
int nvit_attn_bwd_qknorm(int dt, const void* dout, const void* qh, const void* kh, const void* vh, const void* o,
                         const float* lse, float scale, const float* rq, const float* rk, const float* sqk, float c_q,
                         float q_prescale, void* dq, int ldq, void* dk, void* dv, int ldkv, float* part_q, float* part_k,
                         float* delta, int B, int H, int Tq, int Tk, int d, void* stream);

/* ---- head-axis attention (the reference's flash_attn=True branch) -------------------------------------------
 * flash_attn_func reads the reference's [B,H,T,d] tensors as [batch, seqlen, nheads, headdim] (model.py:121-122,252-253,
 * SURVEY §9.1-Q3), so its softmax runs over the H heads of ONE token:
 *   O[m, i*d:(i+1)*d] = sum_j softmax_j(scale * <q~_i, k~_j>) v_j,   i, j < H,  q~_i = (sqk*c_q)_i * nrm(q_i) (sqk != NULL)
 * or q~ = q (sqk == NULL, plain ViT); k~ likewise.  Rows m < M; q [M, ldq], k and v [M, ldkv] fp32 (the projection GEMM
 * outputs, token-major; self-attention: one [M,3C] buffer with ldq = ldkv = 3C).  O [M, C] contiguous, type dt (the A
 * operand of the output projection); lse [M, H] fp32 (natural log of each softmax denominator), the only state the
 * backward needs besides the inputs.  d in {32,64,128}; H <= NVIT_ATTN_HEADS_MAX_H. */
#define NVIT_ATTN_HEADS_MAX_H 32
int nvit_attn_heads_fwd(int dt, const float* q, int ldq, const float* k, const float* v, int ldkv, const float* sqk,
                        float c_q, float scale, void* o, float* lse, int M, int H, int d, void* stream);
/* Backward: dO [M, C] contiguous (type dt) -> dq [M, lddq], dk and dv [M, lddkv] (type dt), the normalise backward
 * included; part_dsqk [nblk, C] fp32 partial sums of d/d(sqk*c_q), one row per workgroup, fixed order (reduce with
 * nvit_colsum_reduce).  sqk == NULL: plain heads, part_dsqk is not written.  nblk in 1..NVIT_ATTN_HEADS_BWD_MAX_BLOCKS
 * workgroups. */
#define NVIT_ATTN_HEADS_BWD_MAX_BLOCKS 8192
int nvit_attn_heads_bwd(int dt, const void* dout, const float* q, int ldq, const float* k, const float* v, int ldkv,
                        const float* sqk, float c_q, float scale, const float* lse, void* dq, int lddq, void* dk,
                        void* dv, int lddkv, float* part_dsqk, int nblk, int M, int H, int d, void* stream);

/* ---- patch embedding / head / reconstruction -------------------------------------------
 * nvit_im2col: A_l [M, ch*Pl*Pl] and A_g [M, ch*Pg*Pg] (type dt, column order (c,ph,pw)) from
 * img fp32 [B,ch,S,S]; global windows are reflect-padded by (Pg-Pl)/2 and strided by Pl
 * (model.py:286-304,407-408).  The exact-fp32 mode multiplies these by the patch weights with nvit_gemm_nt; the
 * bf16 mode never materialises them (nvit_patch_embed_fwd). */
int nvit_im2col(int dt, const float* img, void* A_l, void* A_g, int B, int ch, int S, int Pl, int Pg, void* stream);
/* nvit_patch_embed_fwd: the dual patch embedding of the bf16 mode as ONE kernel (model.py:286-304 the two Conv2d
 * patchifiers, :407-415 their application + position embeddings):
 *   out_l[m] = W_l . patch_l(m) + b_l + pos_l[m % T],   out_g[m] = W_g . patch_g(m) + b_g + pos_g[m % T]   (fp32 [M, C])
 * Patches are gathered from img fp32 [B,ch,S,S] into LDS (same geometry rules as nvit_im2col), split into bf16
 * hi + lo on the fly and multiplied on the bf16 MFMA as hi*hi + lo*hi + hi*lo (fp32-accurate to ~2^-16 relative).
 * w_l / w_g: split weight images [C, 2*Kp] from nvit_shadow_weights (perm 2), Kp = nvit_patch_embed_kp(ch*P*P).
 *   nvit_patch_embed_kp(K) = K rounded up to whole stages of NVIT_PATCH_EMBED_K_STEP patch elements.
 * a_l / a_g: optional bf16 [M rounded up to whole NVIT_PATCH_EMBED_TILE_ROWS, Kp] outputs = the rounded patch rows
 * (columns >= K zero), the saved operand of the weight-gradient GEMM; NULL to skip.  lo_l / lo_g: optional bf16 [M, C]
 * twins of out_l / out_g (the operands of the q and k/v projections; needs C % 8 == 0); NULL to skip.  b_l / b_g may be
 * NULL. */
#define NVIT_PATCH_EMBED_K_STEP 32
#define NVIT_PATCH_EMBED_TILE_ROWS 256
int nvit_patch_embed_kp(int K);
int nvit_patch_embed_fwd(const float* img, const void* w_l, const float* b_l, const float* pos_l, float* out_l, void* lo_l,
                         void* a_l, const void* w_g, const float* b_g, const float* pos_g, float* out_g, void* lo_g,
                         void* a_g, int B, int ch, int S, int Pl, int Pg, int C, void* stream);
/* mean over tokens + LayerNorm(eps) (model.py:455-456, mlp_head.0): x fp32 [B,T,C] ->
 * pooled [B,C] fp32, ln [B,C] fp32 and ln_lo (type dt, ld = C), stats [B,2] = {mean, rstd}. ws [B, nchunk, C]. */
int nvit_pool_ln_fwd(int dt, const float* x, const float* w, const float* b, float eps, float* pooled, float* ln,
                     void* ln_lo, float* stats, float* ws, int nchunk, int B, int T, int C, void* stream);
/* backward of the above: dln [B,C] fp32 -> dx [B,T,C] fp32 (written, broadcast /T), dw, db (+=). */
int nvit_pool_ln_bwd(const float* dln, const float* pooled, const float* w, const float* stats, float* dx,
                     float* dw, float* db, int accumulate, int B, int T, int C, void* stream);
/* recon loss (model.py:459-464): raw fp32 [M, ch*P*P] = x W_r^T + b_r; loss = mean((tanh(raw) - patch(img))^2).
 * part [nblk] partial sums; loss[0] written by a fixed-order final reduce. */
int nvit_recon_loss(const float* raw, const float* img, float* part, int nblk, float* loss, int B, int ch, int S,
                    int P, void* stream);

/* ---- Kohonen (SOM) head, BASELINE config C5 (kohonen.py:100-165, model.py:419-444,482-561) ---------
 * nvit_som_bmu: idx[m] = argmin_n ||x_m - node_n||_2 given scores[M,N] = x . node^T (nvit_gemm_nt, fp32) and the
 *   nodes [N,C] (kohonen.py:111-114 cdist+argmin); nn_ws [N] workspace; first minimum wins.
 * nvit_gather_rows / nvit_scatter_rows: repr = nodes[idx] (kohonen.py:117) and its backward (fixed order).
 * nvit_som_update: KohonenMap.update_nodes (kohonen.py:121-165) for the whole batch, in place on nodes [gm*gn, C]:
 *   B sequential steps; step i uses the BMU of FLAT token i and sample i mean-pooled T*C -> C,
 *   strength lr_alpha * exp(-d2 / (2 sigma^2)), d2 = squared grid distance, wrapped around the map edges when
 *   periodic != 0 (kohonen.py:80-98). v_ws [B,C], s_ws [B,gm*gn].
 * nvit_som_update_dev: the same two launches and arithmetic with lr_alpha read from device memory (1 float, non-NULL)
 *   when the first kernel runs: the entry a captured hipGraph step uses, whose host rewrites the rate between replays
 *   (a by-value argument replays its capture-time value).  Equal rates give the bits of nvit_som_update.
 * nvit_cos_consistency_*: 1 - mean_m cos(a_m, b_m) (model.py:482-491); stats [M,3] saved for backward.
 * nvit_huber_*: F.huber_loss(a, b) with delta 1, mean (model.py:441-442).
 * nvit_som_smooth_*: mean over tokens and 8 periodic grid neighbours of ||node[idx] - node[nb]|| for ONE map
 *   (model.py:503-561); cnt [N] int32 and D [N,8] workspaces are kept for the backward.
 * nvit_recon_bwd: d(raw) of mean((tanh(raw) - patch(img))^2) times g[0] (model.py:459-464), type dt. */
int nvit_som_bmu(const float* scores, const float* nodes, float* nn_ws, int64_t M, int N, int C, int64_t* idx,
                 void* stream);
int nvit_gather_rows(const float* nodes, const int64_t* idx, float* out, int64_t M, int C, void* stream);
int nvit_scatter_rows(const float* dout, const int64_t* idx, float* dnodes, int64_t M, int N, int C, void* stream);
/* out[M,N] fp32 one-hot rows of idx: the balanced form of the scatter is nvit_gemm_tn(onehot, dout) (exact). */
int nvit_onehot(const int64_t* idx, float* out, int64_t M, int N, void* stream);
int nvit_som_update(float* nodes, const float* x, const int64_t* idx, float lr_alpha, float sigma, int gm, int gn,
                    int periodic, float* v_ws, float* s_ws, int B, int T, int C, void* stream);
int nvit_som_update_dev(float* nodes, const float* x, const int64_t* idx, const float* lr_alpha, float sigma, int gm,
                        int gn, int periodic, float* v_ws, float* s_ws, int B, int T, int C, void* stream);
int nvit_cos_consistency_fwd(const float* a, const float* b, float* stats, float* part, int nblk, float* loss,
                             int64_t M, int C, void* stream);
int nvit_cos_consistency_bwd(const float* a, const float* b, const float* stats, const float* g, float* da, float* db,
                             int64_t M, int C, void* stream);
int nvit_huber_fwd(const float* a, const float* b, float* part, int nblk, float* loss, int64_t n, void* stream);
int nvit_huber_bwd(const float* a, const float* b, const float* g, float* da, float* db, int64_t n, void* stream);
int nvit_som_smooth_fwd(const float* nodes, const int64_t* idx, int* cnt, float* D, float* loss, int64_t M, int Nn,
                        int C, int map_size, void* stream);
int nvit_som_smooth_bwd(const float* nodes, const float* D, const int* cnt, const float* g, float* dnodes,
                        int accumulate, int64_t M, int Nn, int C, int map_size, void* stream);
int nvit_recon_bwd(int dt, const float* raw, const float* img, const float* g, void* draw, int B, int ch, int S, int P,
                   void* stream);

/* Loss side: F.cross_entropy(logits, Y) of train.py:906 with its gradient in the same pass.
 * rowloss[B] (workspace) = logsumexp(row) - row[label]; loss[0] = mean; dlogits[B,N] = (softmax - onehot) / B
 * (multiply by the upstream scalar gradient).  Labels outside [0,N) contribute 0 loss (and a plain softmax/B row); the
 * range test is made on the 64-bit label (2^32 + 1 is outside, not class 1), here and in the two entries below. */
int nvit_ce_loss(const float* logits, const int64_t* labels, float* rowloss, float* loss, float* dlogits, int B, int N,
                 void* stream);
/* The same with a soft target (Mixup / CutMix / label smoothing, timm's mixup_target): row b's target is
 * t = (1 - smoothing) * (lam[b] * e[labels[b]] + (1 - lam[b]) * e[labels2[b]]) + smoothing / N; rowloss[b] =
 * logsumexp(row) - (1 - smoothing) * (lam * row[label] + (1 - lam) * row[label2]) - smoothing * mean(row); loss[0] = mean;
 * dlogits = (softmax - t) / B.  lam: device fp32 [B]; 0 <= smoothing < 1.  With lam = 1 and smoothing = 0 the three outputs
 * have the bits of nvit_ce_loss.  A label outside [0,N) contributes no term to the target. */
int nvit_ce_loss_soft(const float* logits, const int64_t* labels, const int64_t* labels2, const float* lam, float smoothing,
                      float* rowloss, float* loss, float* dlogits, int B, int N, void* stream);
/* Evaluation metrics of one batch in one launch (reference train.py:563-575, 595-613): per row the cross-entropy of
 * nvit_ce_loss and rank = #{j : logit_j > logit_y} + #{j < y : logit_j == logit_y} (a label outside [0,N): loss 0,
 * never correct).  NaN logits take the order of torch.topk: a NaN ranks above every number, NaNs tie with each other and
 * the lower index wins.  So a NaN logit that is not the label's outranks the label, and a NaN label logit is a top-1 hit
 * only when no NaN precedes it; the accumulated loss of such a batch is NaN.  ADDS to the device accumulator acc[0..3]: the batch-mean loss, 100 * #(rank < 1) / B,
 * 100 * #(rank < min(5,N)) / B, and 1 (the batch count) - the reference reports means over batches of per-batch
 * values.  Fixed-order reduction, no float atomics: reproducible run to run.  Nothing goes back to the host. */
int nvit_eval_metrics(const float* logits, const int64_t* labels, float* acc, int B, int N, void* stream);

/* ---- gradient all-reduce by direct peer reads over xGMI (nvit/train.py:438-446) --------------
 * Symmetric flat fp32 buffers of n elements (n % 4 == 0), one per rank, mapped into this process (IPC); peer_ptrs is a
 * HOST array of nranks (<= 8) device pointers, [rank] = this rank's own buffer.  chunk = nvit_xgmi_chunk(n, nranks).
 * nvit_xgmi_reduce_scatter: own[rank*chunk ...] = scale * sum over ranks 0..nranks-1 (fixed order) of their chunk `rank`.
 * nvit_xgmi_all_gather   : own[j*chunk ...] = rank j's chunk j, for every j != rank.
 * The caller separates the phases (every rank finished writing / reduce-scatter / all-gather) with its own barrier. */
int64_t nvit_xgmi_chunk(int64_t n, int nranks);
int nvit_xgmi_reduce_scatter(const int64_t* peer_ptrs, int nranks, int rank, int64_t n, float scale, void* stream);
int nvit_xgmi_all_gather(const int64_t* peer_ptrs, int nranks, int rank, int64_t n, void* stream);

/* Device-synchronised form of the same collective (replaces the NCCL communicator the reference's DDP wrapper drives,
 * nvit/train.py:438-446, with phase flags that live on the devices): no host barrier between "gradients written",
 * reduce-scatter and all-gather, several regions ("slots", one per gradient bucket) in flight at once, every call just
 * kernel launches on `stream`.  Each rank owns a flag block in uncached device memory:
 *   nvit_xgmi_flag_bytes(nslots)            size of a flag block (0 for a bad slot count; at most 64 slots)
 *   nvit_xgmi_flags_alloc(nslots, &p, h)    allocate + zero this rank's block, h = 64-byte IPC handle to send to the peers
 *   nvit_xgmi_flags_open(h, &p) / _close(p) map / unmap a peer's block;  nvit_xgmi_flags_free(p) frees the own block
 *   nvit_xgmi_flags_error(own, nslots, &w, stream)   synchronises `stream`, w = 0 or (code << 8 | slot + 1) of the first
 *                                           wait that timed out ON ANY RANK: 1 reduce-scatter, 2 all-gather, 3 wait_gathered
 *   nvit_xgmi_set_timeout(seconds)          bound of every device-side wait (default 1800 s = the reference's 30-minute
 *                                           process-group timeout, train.py:224); set the same value on every rank
 *   nvit_xgmi_errword_alloc(&host, &dev) / _free(host)   one pinned host word the device can write
 * A timeout is fatal and fails closed: the timing-out rank stores the error word into EVERY rank's flag block, waits give
 * up as soon as their own error word is set, a kernel whose wait failed moves no data and announces no phase (nobody
 * gathers an unreduced chunk), and nvit_xgmi_wait_gathered copies the error word to the pinned host word it is given, so
 * the host can check it after every step without synchronising.
 * flag_ptrs: HOST array of nranks device pointers to the flag blocks ([rank] = own).  Region = elements [off, off + n) of
 * every symmetric buffer (multiples of 4), chunked by nvit_xgmi_chunk(n, nranks); `epoch` = number of this call for the
 * slot, from 1, the same on every rank.  A region may be rewritten only after nvit_xgmi_wait_gathered has been enqueued
 * for its slot (slots / epochs: HOST arrays of nwait <= 64 entries, passed to the kernel by value; host_err_dev: the
 * device pointer from nvit_xgmi_errword_alloc, or NULL) on the stream that rewrites it. */
int64_t nvit_xgmi_flag_bytes(int nslots);
int nvit_xgmi_flags_alloc(int nslots, void** dev_ptr, void* ipc_handle_out);
int nvit_xgmi_flags_open(const void* ipc_handle, void** dev_ptr);
int nvit_xgmi_flags_close(void* dev_ptr);
int nvit_xgmi_flags_free(void* dev_ptr);
int nvit_xgmi_flags_error(const void* own_flags, int nslots, unsigned* out, void* stream);
int nvit_xgmi_reduce_scatter_sync(const int64_t* peer_ptrs, const int64_t* flag_ptrs, int nranks, int rank, int nslots,
                                  int slot, unsigned epoch, int64_t off, int64_t n, float scale, void* stream);
int nvit_xgmi_all_gather_sync(const int64_t* peer_ptrs, const int64_t* flag_ptrs, int nranks, int rank, int nslots, int slot,
                              unsigned epoch, int64_t off, int64_t n, void* stream);
int nvit_xgmi_wait_gathered(const int64_t* flag_ptrs, int nranks, int rank, int nslots, const int* slots,
                            const unsigned* epochs, int nwait, void* host_err_dev, void* stream);
int nvit_xgmi_set_timeout(double seconds);
int nvit_xgmi_errword_alloc(void** host_ptr, void** dev_ptr);
int nvit_xgmi_errword_free(void* host_ptr);

/* Attention backward, dK/dV kernel: 1 = the hand-placed (generated-assembly) main loop where it applies (pre-scaled q,
 * the fused entry point; default), 0 = the compiler-built kernel.  Both compute bit-identical results
 * (tests/test_gpu_ops.py). */
int nvit_set_attn_dkv_asm(int on);

#ifdef __cplusplus
}
#endif
#endif /* NVIT_HIP_H */

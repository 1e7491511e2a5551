/* C ABI of libtvts_hip.so -- the MI355X (gfx950) kernels under the TVTSv2 pretrain step.
 *
 * The reference (TencentARC/TVTS v2) has no FFI: its hot path is stock PyTorch ops.
 * Each entry point below replaces the ATen op(s) at the cited reference site; INTEGRATION.md shows the
 * ctypes binding a maintainer adds.  Conventions: raw device pointers, explicit sizes / leading
 * dimensions in ELEMENTS, asynchronous on `stream`, no allocation inside, re-entrant, return 0 or a
 * hipError_t (> 0) / -22 for an invalid argument.  bf16 = 16-bit brain float, row-major everywhere.
 *
 * The library keeps NO mutable process state: entry points are called from the main thread, from PyTorch's autograd worker
 * thread and from communication hooks.  Where a kernel family has alternative dispatch paths (tile sizes, split
 * counts, fused / split passes) the entry point takes a per-call `opts` word -- 0 is the automatic choice the training step
 * uses, the TVTS_*  bits below select the alternatives for parity tests and benches (tests/test_abi.py::test_two_threads).
 */
#ifndef TVTS_HIP_H
#define TVTS_HIP_H
#include <hip/hip_runtime_api.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { TVTS_ACT_NONE = 0, TVTS_ACT_QUICK_GELU = 1, TVTS_ACT_GELU_ERF = 2,
       TVTS_GATE_ADD_BF16 = 3 /* gate_act only: gate_h is a bf16 matrix ADDED to the result -- the bf16 residual stream */ };
enum { TVTS_ATTN_FULL = 0, TVTS_ATTN_SPACE = 1, TVTS_ATTN_TIME = 2, TVTS_ATTN_CLS = 3 };
/* `opts` of the GEMM entry points (OR them; 0 = automatic) */
enum {
    TVTS_GEMM_TILE_128 = 1,     /* force the persistent 128x128 kernel */
    TVTS_GEMM_TILE_256 = 2,     /* force the pipelined 256x256 kernel: -22 if ldc / ldp / ldh is not a multiple of 8 (its 16-byte epilogue
                                   accesses); a result with N % 8 != 0 is not this kernel's to take and runs on the 128x128 one
                                   (tvts_gemm_nt_select reports 128 for it) */
    TVTS_GEMM_FP8_K32 = 4,      /* tvts_gemm_nt_fp8*: the 16x16x32 fp8 MFMA main loop (bf16 issue rate) instead of the K = 128 scaled
                                   MFMA; both accumulate the same products in fp32 */
    TVTS_TN_NO_EARLY_DMA = 4,   /* tvts_gemm_tn_bf16: LDS-DMA through the builtin path (the one operands past 4 GiB take) */
    TVTS_TN_AFAST_0 = 8,        /* tvts_gemm_tn_bf16: tile walk of an m-range, b-dimension fastest ... */
    TVTS_TN_AFAST_1 = 16,       /* ... or a-dimension fastest (default: the shorter one) */
    TVTS_GEMM_STREAMK = 32,     /* tvts_gemm_nt_bf16 / tvts_gemm_tn_bf16: force the stream-K walk (work split by K stage, ordered sum of the
                                   partial tiles in the block that arrives last); -22 without a workspace or on a shape it cannot take (one K stage, fewer
                                   than 8 tiles, and -- the walk exists on the 256x256 kernel only -- ldc / ldp / ldh not a multiple of 8) */
    TVTS_GEMM_NO_STREAMK = 64,  /* ... never take it */
    TVTS_GEMM_RING = 128,       /* tvts_gemm_nt_bf16: force the ring form of the 128-column kernel (one block per CU, three 64-deep stages
                                   in flight: the small-batch kernel; same bits as TVTS_GEMM_TILE_128); -22 if an operand is too large
                                   for its 32-bit offsets.  Automatic where its cost model wins (csrc/gemm.hip, nt_use_ring) */
    TVTS_GEMM_NO_RING = 16384,  /* ... never take it */
    TVTS_GEMM_F32_PATCH = 4194304,   /* tvts_gemm_nt_bf16, 256 x 256 kernel, plain bf16 results (round 6): the fp32 LDS patch of the epilogue instead of the
                                   bf16-first patch (the tile rounded in the accumulator layout, two 16-row slabs per 4 KiB patch) -- the same
                                   bits either way (tests/test_bench_path_gpu.py), the old kernel for A/Bs */
    TVTS_GEMM_CLOCK_SAMPLE = 2097152, /* tvts_gemm_nt_bf16, plain bf16 result on the 256 x 256 kernel (round 6, bench.py's instrumented step): block 0
                                   writes {s_memtime, s_memrealtime} at its first instruction and behind its last tile into the LAST 32 bytes
                                   of `workspace` (4 x u64: cycles0, ticks0, cycles1, ticks1) -- shader cycles over constant-rate ticks =
                                   the clock the launch ran at.  A separate instantiation: the kernels of every other call are unchanged;
                                   ignored where the call takes another kernel or the stream-K walk */
    TVTS_GEMM_SIDE_DERIV = 1048576 /* tvts_gemm_nt_bf16 / _fp8 / _fp8_gate (round 5): the activation forms store act'(x) in `preact` instead of the
                                   pre-activation x, the gate forms take `gate_h` as that derivative and multiply by it as is -- the forward
                                   epilogue evaluates the sigmoid / erf parts anyway, the input-gradient epilogue then needs no
                                   transcendental at all.  Both GEMMs of an MLP must agree on it (the stored tensor changes meaning). */
};
/* measurement hook: tile rows of the forced ring kernel, 128 / 192 / 256 (0 = its own choice between 128 and 192) */
#define TVTS_GEMM_RING_ROWS(r) ((r) == 128 ? (1 << 16) : (r) == 192 ? (2 << 16) : (r) == 256 ? (3 << 16) : 0)
/* persistent grid of the 256x256 NT kernels (bf16 and fp8): at most n blocks, one per CU (8 .. 256, multiple of 8; 0 = the whole
 * chip) -- leaves CUs to kernels of other streams (the RCCL kernels of the side stream when world > 1), and a measurement
 * hook (tools/gemm_cus.py) */
#define TVTS_GEMM_CUS(n) ((((n) / 8) & 63) << 8)
/* tvts_gemm_tn_bf16: number of contraction ranges (0 = automatic: the smallest count that fills >= 93 % of a round) */
#define TVTS_TN_SPLITS(s) ((s) << 8)
/* `opts` of the attention entry points */
enum {
    TVTS_ATTN_NO_TR = 1,        /* scalar LDS reads instead of ds_read_b64_tr_b16 fragments */
    TVTS_ATTN_NO_SHARED = 2,    /* per-wave instead of block-shared K / V (Q / dO) staging */
    TVTS_ATTN_NO_FUSED = 4      /* the split passes instead of the fused single-launch kernels */
    /* bits 4..6 (tvts_attn_bwd only): timing ablations of the fused backward, results wrong by construction */
};

/* ---- GEMM (gemm.hip).  nn.Linear forward / dgrad: v2/model/video_encoder_ViT_B_16.py:26-27,41,74,105-109;
 *      v2/CLIP/clip/model.py:175-181; v2/model/sort_transformer.py:21-23,41-42.  K % 64 == 0, N % 4 == 0.
 *      out = [gate'(gate_h) *] act(A.B^T + bias) [+ residual]; preact (bf16) receives A.B^T + bias when act != 0.
 *      gate_act = TVTS_GATE_ADD_BF16: out = A.B^T + bias + gate_h (bf16 residual: x + proj(.) / x + mlp(.) of
 *      video_encoder_ViT_B_16.py:117-123 with the residual stream kept in bf16; `residual` is the fp32 form of the same sum)
 *      workspace (optional, workspace_bytes >= tvts_gemm_nt_workspace_bytes()): scratch of the stream-K walk the entry point
 *      takes when an output of few tiles would leave the persistent grid a fraction of a round (the reference's own per-GPU
 *      batches of 12 / 24 pairs): fp32 partial tiles + one arrival counter per output tile.  Its first 64 KiB must be ZERO
 *      on the first call and are zero again after every call; one workspace serves one stream (calls in flight at the same
 *      time need workspaces of their own).  Without it the tile-granular walk is the only one.
 *      Refused with -22 before any launch: a null A / B / out, M / N / K <= 0, K % 64, N % 4, lda / ldb % 8, ldc / ldr / ldp / ldh % 4
 *      (% 8 for ldc / ldp / ldh under TVTS_GEMM_TILE_256), a leading dimension shorter than its row -- lda < K, ldb < K, ldc < N, and
 *      ldr / ldp / ldh < N when that matrix is given (so 0, a broadcast row, is refused: no caller passes one) --, act together with
 *      gate_h, workspace_bytes < 0. */
int tvts_gemm_nt_bf16(const void* A, int lda, const void* B, int ldb, int M, int N, int K, const float* bias,
                      const float* residual, int ldr, int act, void* preact, int ldp, const void* gate_h, int ldh,
                      int gate_act, void* out, int ldc, int out_f32, void* workspace, long workspace_bytes, int opts,
                      hipStream_t stream);
long tvts_gemm_nt_workspace_bytes(void);
/* the kernel tvts_gemm_nt_bf16 picks for an [M, N] result under `opts` -- 256 / 128 = the output tile of the pipelined / the
 * double-buffered kernel, 1128 / 1192 = the ring kernel (TVTS_GEMM_RING) with 128 / 192 tile rows: lets a parity test assert that
 * the kernel it means to exercise is the one that ran */
int tvts_gemm_nt_select(int M, int N, int opts);
/* weight gradient: out[Na,Nb] (+)= P[M,Na]^T . Q[M,Nb], bf16 in, fp32 out (autograd of the Linear sites above).
 * Refused with -22 before any launch: a null P / Q / out, M / Na / Nb <= 0, Na / Nb / ldp / ldq % 8, ldo % 4, ldp < Na, ldq < Nb,
 * ldo < Nb, workspace_elems < 0. */
/* colsum (optional): colsum[a] += sum_m P[m,a] -- the bias gradient, fused into the same pass.
 * workspace (optional, workspace_elems floats): scratch for the split-M partials; with it the kernel stores
 * partials that are combined in range order (deterministic), without it the partials meet through fp32 atomics.
 * counters (optional, n_counters ints, ZERO on the first call and zero again after every call; one array per stream): with them
 * and TVTS_GEMM_STREAMK in `opts` the block that arrives last at an output tile adds that tile's partials itself (same order, same
 * bits as the separate reduce pass, one launch less -- and measured slower: the partials then travel at agent scope and one block
 * sums them); otherwise a reduce pass follows the kernel. */
int tvts_gemm_tn_bf16(const void* P, int ldp, const void* Q, int ldq, int M, int Na, int Nb, float* out, int ldo,
                      int accumulate, float* colsum, float* workspace, long workspace_elems, int* counters, int n_counters,
                      int opts, hipStream_t stream);
/* Several weight gradients in ONE launch + ONE ordered reduce launch (the six of a ViT block at the reference's per-GPU batches, where
 * each alone fills a fraction of a round): problems = HOST array of n records
 *   struct { const void* P; int ldp; const void* Q; int ldq; int M, Na, Nb; float* out; int ldo; int accumulate; float* colsum; }
 * (the arguments of tvts_gemm_tn_bf16); table_dev = device memory for the plan (tvts_gemm_tn_grouped_table_bytes(n)), table_host = HOST
 * staging memory of the same size, owned by the caller (page-locked, so that the copy is truly asynchronous) and left untouched until
 * the stream has passed this call.  upload != 0 builds the plan in table_host and copies it with ONE hipMemcpyAsync on `stream`, in
 * front of the kernels that read it -- no host wait, ordered on whatever stream the caller launches on; upload == 0 re-uses the plan a
 * previous call with the SAME problems and workspace left in table_dev (table_host may be NULL).  Every problem's result has the bits
 * of tvts_gemm_tn_bf16 called with the same range count.
 * Refused with -22 before any launch: n <= 0 or n > 64, a null problems / table_dev / workspace, table_bytes short, upload without
 * table_host, a record tvts_gemm_tn_bf16 would refuse (null P / Q / out, M / Na / Nb <= 0, Na / Nb / ldp / ldq % 8, ldo % 4, ldp < Na,
 * ldq < Nb, ldo < Nb), a workspace too small for the partials of the ranges. */
int tvts_gemm_tn_bf16_grouped(const void* problems, int n, void* table_dev, void* table_host, long table_bytes, int upload,
                              float* workspace, long workspace_elems, int opts, hipStream_t stream);
long tvts_gemm_tn_grouped_table_bytes(int n);
/* the tile (128: 128x128 kernel, two blocks per CU; 256: pipelined 256x256 kernel) tvts_gemm_tn_bf16 picks for M rows into an
 * [Na, Nb] output under `opts` */
int tvts_gemm_tn_select(int M, int Na, int Nb, int opts);
/* fp8 (OCP e4m3) operands with scales in device memory, fp32 accumulate: the GEMM of BASELINE config 4's weight / activation
 * path (nn.Linear sites of video_encoder_ViT_H_14.py); K % 128 == 0, lda / ldb % 16 == 0 (bytes).  scale_b: one scale for the
 * weight; scale_a: one scale for the tensor, or (scale_a_rows != 0) M per-row scales as written by tvts_quant_fp8_rows.
 * Refused with -22 before any launch (here and in tvts_gemm_nt_fp8_gate): a null A / B / scale, sizes <= 0, K % 128, N % 8,
 * lda / ldb % 16, ldc / ldp / ldh / ldq8 % 8, ldr % 4, lda < K, ldb < K, and ldc / ldr / ldp / ldh / ldq8 < N for every matrix given */
int tvts_gemm_nt_fp8(const void* A, int lda, const void* B, int ldb, int M, int N, int K, const float* scale_a,
                     int scale_a_rows, const float* scale_b, const float* bias, const float* residual, int ldr, int act, void* preact, int ldp,
                     void* out, int ldc, int out_f32, void* q8out, int ldq8, const float* q8_scale, float* q8_amax, int opts,
                     hipStream_t stream);
/* q8out (optional; activation forms with a bf16 result, here and in tvts_gemm_nt_fp8_gate): the epilogue also writes
 * q8out[m, n] = e4m3(out[m, n] / q8_scale[0]) and folds max |out| into q8_amax -- the per-tensor copy the next GEMMs of
 * BASELINE config 5 read (the following layer's forward and weight gradient), without a quantiser pass over the result.  With q8out,
 * `out` may be NULL: the e4m3 copy is then the only result (round 5: in the per-tensor regime nothing reads the bf16 tensor) */
/* input gradient of such a layer (autograd of nn.Linear + the GELU of video_encoder_ViT_H_14.py's Mlp): out[M,N] (bf16) =
 * gate_act'(gate_h[M,N]) * (scale_a[m] * scale_b * (A[M,K] B[N,K]^T)), A = e4m3 copy of the output gradient (per-token scales),
 * B = e4m3 copy of the transposed weight; the un-gated input gradients take tvts_gemm_nt_fp8 itself */
int tvts_gemm_nt_fp8_gate(const void* A, int lda, const void* B, int ldb, int M, int N, int K, const float* scale_a,
                          int scale_a_rows, const float* scale_b, const float* bias, const void* gate_h, int ldh, int gate_act,
                          void* out, int ldc, void* q8out, int ldq8, const float* q8_scale, float* q8_amax, int opts,
                          hipStream_t stream);
/* weight gradient of such a layer on e4m3 operands: out[Na,Nb] (+)= scale_p * scale_q * sum_m P8[m,Na] * Q8[m,Nb].  The contraction runs
 * over the tokens, so the operands carry ONE scale per tensor (device scalars; tvts_quant_fp8 / tvts_quant_fp8_rows2 write such
 * copies) -- not the per-token scales of the forward / input-gradient operands.  Na, Nb, ldp, ldq (bytes) multiples of 16;
 * -22 also for a null P8 / Q8 / out / scale, ldp < Na, ldq < Nb, ldo < Nb, workspace_elems < 0.
 * workspace: split-M partials, reduced in range order (deterministic).  colsum (optional): colsum[a] += scale_p * sum_m P8[m,a] --
 * the bias gradient from the SAME e4m3 bytes the weight gradient is made of (a ones operand on the matrix pipe). */
int tvts_gemm_tn_fp8(const void* P8, int ldp, const void* Q8, int ldq, int M, int Na, int Nb, const float* scale_p,
                     const float* scale_q, float* out, int ldo, int accumulate, float* colsum, float* workspace,
                     long workspace_elems, int opts, hipStream_t stream);
/* (main loop of tvts_gemm_nt_fp8*: v_mfma_scale_f32_16x16x128_f8f6f4 with unit scales, the fp8 issue rate of gfx950;
 * TVTS_GEMM_FP8_K32 selects the 16x16x32 fp8 form.  Both e4m3 instructions leave an error of about 2^-12 of an element's largest
 * product whatever the contraction length, which only a long contraction's fp32-accumulation bound covers: contractions shorter
 * than 512 -- K of tvts_gemm_nt_fp8 / _fp8_gate, M of tvts_gemm_tn_fp8 -- run with the e4m3 values decoded to bf16 in registers
 * (exact) on the bf16 MFMA, whichever main loop `opts` names) */
/* per-tensor fp8 quantisation: amax[0] = max |x| ; q = rne(x * 448 / amax) as e4m3, scale_out[0] = amax / 448.
 * Refused with -22 before any launch (here, in tvts_quant_fp8_rows, tvts_quant_fp8_multi and tvts_fp8_update_scales): rows / cols /
 * n <= 0, cols % 8 (bf16) or % 4 (fp32), ld off a 16-byte multiple, ldo % 8, ld or ldo < cols with more than one row, a null x / out /
 * amax / table / scale, and tvts_quant_fp8_rows with neither row_scale nor tscale */
int tvts_amax(const void* x, int is_f32, long ld, int rows, int cols, float* amax, hipStream_t stream);
int tvts_quant_fp8(const void* x, int is_f32, long ld, int rows, int cols, const float* amax, void* out, long ldo,
                   float* scale_out, hipStream_t stream);
/* the same for MANY weights in three launches (every fp8 weight of the model, once per optimizer step).  table: n device records
 *   struct { const float* w; uint8_t* q; const bf16* wt; uint8_t* qt; float* amax; float* scale; float* scale_t; int rows, cols; }
 * w = fp32 master [rows, cols] contiguous, q its e4m3 copy; wt (optional) the bf16 transposed copy [cols, rows] and qt its e4m3
 * copy under the SAME scale (amax of the master); rows * cols % 4 == 0 */
int tvts_quant_fp8_multi(const void* table, int n, hipStream_t stream);
/* per-row (per-token) quantisation of a bf16 activation in one pass: row_scale[r] = amax(x[r,:]) / 448 (1 for an all-zero
 * row), out[r,:] = e4m3(x[r,:] / row_scale[r]); cols % 8 == 0 */
int tvts_quant_fp8_rows(const void* x, long ld, int rows, int cols, void* out, long ldo, float* row_scale,
                        const float* tscale, float* amax_acc, hipStream_t stream);
/* Per-tensor (delayed) scaling -- the form the e4m3 WEIGHT GRADIENT needs, whose contraction over the tokens cannot carry per-token
 * scales: with tscale (device scalar) every row is quantised under that one scale instead of its own amax / 448 (row_scale may then be
 * null), so the same bytes serve tvts_gemm_nt_fp8* (scale_a = tscale, scale_a_rows = 0) and tvts_gemm_tn_fp8; amax_acc (device scalar,
 * optional, in either mode) receives max(amax_acc, max |x|) of the call.  tvts_fp8_update_scales turns a step's amax values into the
 * next step's scales: scale[i] = amax[i] / 448 where amax[i] > 0, amax[i] = 0.  The same two arguments exist on the LayerNorm forms
 * below. */
int tvts_fp8_update_scales(float* amax, float* scale, int n, hipStream_t stream);
/* The update under the overflow guard of the pretraining step: a maximum that is not finite never becomes a scale.  Per slot:
 * amax[i] finite and > 0: scale[i] = amax[i] / 448; anything else (0, -0, inf, NaN): scale[i] is kept.  A slot whose scale is then
 * not finite and positive -- it has never had a usable maximum (the calibration step was the bad one), or the quotient underflowed
 * -- is set to 1.0, the value the quantisers use at a zero scale, so no quantiser ever divides by 0, inf or NaN.  amax[i] = 0 in
 * every case.  guard_norm (optional device scalar, 4-byte aligned): the step's global gradient norm (norm_coef[0] of
 * tvts_grad_sumsq); when it is not finite -- a step the guarded optimizer skips -- every slot keeps its old scale (the 1.0 rule
 * still applies), so the scales are those of the last step that counted.  -22: n <= 0, amax or scale null, guard_norm misaligned. */
int tvts_fp8_update_scales_guarded(float* amax, float* scale, int n, const float* guard_norm, hipStream_t stream);
/* strided fp32 matmul for the tiny products (text_projection model_dist..B_16.py:108, head sort_transformer.py:113,
 * sim_matrix model_dist..B_16.py:126): C[i,j] (+)= alpha * sum_k A[i*sai+k*sak] * B[k*sbk+j*sbj] + bias[j] */
int tvts_gemm_small_f32(const float* A, long sai, long sak, const float* B, long sbk, long sbj, int M, int N, int K,
                        float alpha, const float* bias, float* C, long ldc, int accumulate, hipStream_t stream);
/* a FEW rows through a linear layer with fp32 result and fp32 residual: out[r, n] = residual[r, n] + bias[n] + sum_k A[r * lda + k] W[n * ldw + k]
 * (A, W bf16; N % 16 == 0, K % 32 == 0, lda / ldw % 8 == 0 and >= K, ldo >= N, ldr >= N with a residual, else -22; bias / residual
 * optional).  The CLS rows of the hybrid residual stream through the blocks'
 * residual-adding projections (`x + attn(...)`, `x + mlp(...)`, video_encoder_ViT_B_16.py:121-124): one row per clip, lda = S * K. */
int tvts_rows_linear_bf16(const void* A, long lda, const void* W, int ldw, int R, int N, int K, const float* bias, const float* residual,
                          int ldr, float* out, int ldo, hipStream_t stream);
/* the same rows on e4m3 operands: out[r, n] = residual[r, n] + bias[n] + row_scale[r] * w_scale[0] * sum_k A8[r * lda + k] W8[n * ldw + k]
 * (A8, W8 OCP e4m3 bytes; row_scale[R] as tvts_quant_fp8_rows writes it, w_scale the weight's device scalar; fp32 accumulation in a
 * fixed order; K % 64 == 0, lda / ldw % 16 == 0 (bytes), both base addresses 16-byte aligned, any N; bias / residual optional).  The
 * CLS rows of the forward-only encoder's last block on an e4m3 architecture: the products of attn.proj / mlp.c_proj that the training
 * forward forms on the e4m3 copies for every row (nn.Linear sites of video_encoder_ViT_H_14.py), one row per clip, lda = S * K. */
int tvts_rows_linear_fp8(const void* A8, long lda, const float* row_scale, const void* W8, int ldw, const float* w_scale, int R, int N,
                         int K, const float* bias, const float* residual, int ldr, float* out, int ldo, hipStream_t stream);
/* bias gradient: out[n] += sum_m X[m,n].  workspace (optional): partial sums of row ranges, added in range order (deterministic, and
 * a grid over the rows as well as the columns); without it one block per 64 columns walks every row.  N % 8 == 0, ld % 8 == 0,
 * ld >= N, X / out not null, workspace_elems >= 0, else -22 */
int tvts_colsum_bf16(const void* X, int ld, int M, int N, float* out, float* workspace, long workspace_elems, hipStream_t stream);

/* ---- LayerNorm (norm.hip): video_encoder_ViT_B_16.py:79-85 (eps 1e-5), sort_transformer.py:99 (eps 1e-6)
 * Refused with -22, by every entry point below, before anything is launched: M <= 0; W <= 0, W % 4, W > 1280; a leading dimension of
 * a matrix that is given (x, y, q8, dy, res1, res2, dx, dx_bf16) that is not a multiple of 4 or is shorter than the row (ld < W: rows
 * would overlap); an absent optional matrix passes ld = 0.  x, gamma, beta must not be NULL, nor dy, mean, rstd in the backward forms
 * (the forward's mean / rstd outputs are optional); tvts_layernorm_fwd needs y.  dgamma and dbeta are given together or not at all;
 * workspace_elems >= 0.  bf16 x takes no fp32 y, no fp32 dy and no fp32 res1; q8 needs row_scale or tscale; res2 needs res1 in the
 * fp8 and cls backward forms; cls_period > 0 and M % cls_period == 0. */
int tvts_layernorm_fwd(const void* x, int ldx, int x_bf16, const int* rows, const float* gamma, const float* beta, float eps, int M,
                       int W, void* y, int ldy, int y_f32, float* mean, float* rstd, hipStream_t stream);
/* the same, additionally writing the bf16 output as OCP e4m3 bytes q8[M, W] (ldq bytes per row) with one scale per row
 * (row_scale[M] = amax(row) / 448): the fp8 operand of the GEMM that follows (BASELINE config 4), identical to
 * tvts_quant_fp8_rows run on y.  y may be NULL (bf16 x, W % 8 == 0, W <= 1536, ldx % 8 == ldq % 8 == 0): the e4m3 bytes are
 * then the only output -- under per-tensor scales (tscale) the GEMMs that follow never read the bf16 tensor.  The same holds
 * for tvts_layernorm_fwd_cls with q8. */
int tvts_layernorm_fwd_fp8(const void* x, int ldx, int x_bf16, const int* rows, const float* gamma, const float* beta, float eps,
                           int M, int W, void* y, int ldy, void* q8, int ldq, float* row_scale, const float* tscale, float* amax_acc,
                           float* mean, float* rstd, hipStream_t stream);
/* dx = LayerNorm backward (+ res1 + res2): res1 is the residual-stream gradient, fp32 or (res1_bf16 != 0, bf16 dy only) bf16 --
 * the space-time block's backward carries it in bf16, the precision its GEMM consumers read it in anyway; res2 a bf16 side branch */
int tvts_layernorm_bwd(const void* dy, int lddy, int dy_f32, const void* x, int ldx, int x_bf16, const int* rows, const float* mean,
                       const float* rstd, const float* gamma, const void* res1, int res1_bf16, int ldr, const void* res2_bf16, int ldr2,
                       int M, int W, float* dx, int lddx, void* dx_bf16, int lddxb, float* dgamma, float* dbeta,
                       float* workspace, long workspace_elems, hipStream_t stream);
/* the same with the e4m3 copy of dx_bf16 (one scale per row, the bytes tvts_quant_fp8_rows would write): the output gradient of the
 * e4m3 input-gradient GEMM that consumes dx_bf16.  bf16 dy, every row, dx_bf16 required; x fp32 with res1 / res1 + res2 / no
 * residual, or x bf16 without residuals */
int tvts_layernorm_bwd_fp8(const void* dy, int lddy, const void* x, int ldx, int x_bf16, const float* mean, const float* rstd,
                           const float* gamma, const void* res1, int res1_bf16, int ldr, const void* res2_bf16, int ldr2, int M, int W, float* dx,
                           int lddx, void* dx_bf16, int lddxb, void* q8, int ldq, float* row_scale, const float* tscale, float* amax_acc,
                           float* dgamma, float* dbeta, float* workspace, long workspace_elems, hipStream_t stream);
/* The HYBRID residual stream of the space-time blocks (round 5; replaces the fp32 activations `x + ...` of
 * video_encoder_ViT_B_16.py:113-124 byte for byte except one row per clip): the stream x [M, W] is bf16, but the row of each clip's CLS
 * token (rows r % cls_period == 0) -- the row the video embedding is read from, and the one row whose rounding error reaches every
 * other token through the attention -- is carried in fp32 in a compact side array cls_x [M / cls_period, W].  Forward: those rows are
 * normalised from cls_x (their stream rows are stale) and x_refresh (normally x itself, optional) receives their bf16 rounding, so that
 * later readers of the stream see the exact value rounded once.  q8 .. amax_acc optional, as in tvts_layernorm_fwd_fp8. */
int tvts_layernorm_fwd_cls(const void* x, int ldx, const float* cls_x, int cls_period, void* x_refresh, const float* gamma,
                           const float* beta, float eps, int M, int W, void* y, int ldy, void* q8, int ldq, float* row_scale,
                           const float* tscale, float* amax_acc, float* mean, float* rstd, hipStream_t stream);
/* Backward on the hybrid stream: bf16 dy, bf16 x, every row; res1_bf16 (optional) the bf16 stream gradient, res2_bf16 (optional, with
 * res1) a bf16 side branch; dx_bf16 required.  Rows r % cls_period == 0: input from cls_x (optional), stream gradient from cls_res1
 * (optional, fp32 [M / cls_period, W]) instead of res1's row, result ALSO to cls_dx (optional, fp32) -- the CLS token's gradient chain
 * never passes through a bf16 rounding.  q8 .. amax_acc optional, as in tvts_layernorm_bwd_fp8; amax_acc receives the maximum of the
 * dx_bf16 that is left behind: what the plain launch forms on the CLS rows from the stream's own rows, and the CLS launch replaces, is
 * kept out of it. */
int tvts_layernorm_bwd_cls(const void* dy, int lddy, const void* x, int ldx, const float* cls_x, const float* cls_res1, float* cls_dx,
                           int cls_period, const float* mean, const float* rstd, const float* gamma, const void* res1_bf16, int ldr,
                           const void* res2_bf16, int ldr2, int M, int W, void* dx_bf16, int lddxb, void* q8, int ldq, float* row_scale,
                           const float* tscale, float* amax_acc, float* dgamma, float* dbeta, float* workspace, long workspace_elems,
                           hipStream_t stream);

/* ---- attention (attention.hip), head dim 64, packed qkv [rows, 3*heads*64]:
 *      divided space-time attention video_encoder_ViT_B_16.py:11-15,38-76; causal text attention
 *      CLIP/clip/model.py:185-187,330-336; sort-head attention sort_transformer.py:45-53 */
int tvts_attn_fwd(int mode, const void* qkv, int ld, int B, int heads, int S, int T, int n, int causal, void* out, int ldo,
                  float* lse2, int opts, hipStream_t stream);
int tvts_attn_delta(const void* dO, int lddo, const void* O, int ldo, int rows, int heads, float* delta,
                    hipStream_t stream);
int tvts_attn_bwd_dq(int mode, const void* qkv, int ld, int B, int heads, int S, int T, int n, int causal, const void* dO,
                     int lddo, const float* lse2, const float* delta, void* dqkv, int lddq, int opts, hipStream_t stream);
int tvts_attn_bwd_dkv(int mode, const void* qkv, int ld, int B, int heads, int S, int T, int n, int causal, const void* dO,
                      int lddo, const float* lse2, const float* delta, void* dqkv, int lddq, float* cls_acc, int opts,
                      hipStream_t stream);
int tvts_attn_cls_finalize(const float* cls_acc, int B, int heads, int S, void* dqkv, int lddq, hipStream_t stream);
/* whole backward of one attention site (D = rowsum(dO*O), dQ, dK, dV, CLS query + CLS key/value reduction of the divided
 * geometries) = the autograd of VarAttention.forward video_encoder_ViT_B_16.py:38-76; delta [rows, heads] and
 * cls_acc (cls_acc_elems fp32 elements) are scratch.  SPACE groups of <= 112 tokens run as ONE fused launch.  cls_acc holds the
 * CLS token's dK / dV / dQ shares: with >= B * heads * max(T, ceil(n / 28)) * 3 * dh elements every block of the fused kernels
 * stores its share and they are added in a fixed order (run-to-run reproducible); with B * heads * 3 * dh elements (the
 * minimum) the shares are accumulated with fp32 atomics. */
int tvts_attn_bwd(int mode, const void* qkv, int ld, int B, int heads, int S, int T, int n, int causal, const void* dO,
              int lddo, const void* O, int ldo, const float* lse2, float* delta, void* dqkv, int lddq, float* cls_acc,
              long cls_acc_elems, int opts, hipStream_t stream);
/* forward of one divided-attention site including the CLS row (VarAttention.forward video_encoder_ViT_B_16.py:38-76);
 * cls_ws: fp32 scratch of >= B * heads * max(T, ceil(n / 28)) * (dh + 2) elements (partial softmax states of the CLS query).
 * lse2 == NULL (here and in tvts_attn_fwd of every mode, tvts_attn_fwd_rowq, tvts_attn_fwd_tail; dh 64 and 80): a forward-only
 * call that stores no log-sum-exp (the inference encoders); with lse2 given nothing changes.  Forward-only SPACE calls with
 * 112 < n + 1 <= 272 (full frames: n = 196, 256) run a fused kernel of their own -- a block per (clip, head, frame), the group's
 * K / V in LDS once, the CLS row from the per-frame partial states -- instead of the streaming kernel + the CLS-query pass. */
int tvts_attn_fwd_divided(int mode, const void* qkv, int ld, int B, int heads, int S, int T, int n, void* out, int ldo,
                      float* lse2, float* cls_ws, long cls_ws_elems, int opts, hipStream_t stream);
/* the two site entry points with the per-tensor e4m3 copy of their result written by the kernels themselves (BASELINE config 5: the
 * attention output feeds the projection's forward and weight-gradient GEMMs, dqkv the qkv projection's input- and weight-gradient
 * GEMMs): q8out[r, c] = e4m3(result[r, c] / q8_scale[0]) with the result's leading dimension (ldq8 == ldo resp. lddq, in bytes),
 * q8_amax = max(q8_amax, max |result|).  Fused geometries only (SPACE n + 1 <= 112, TIME T + 1 <= 32), -22 otherwise. */
int tvts_attn_fwd_divided_q8(int mode, const void* qkv, int ld, int B, int heads, int S, int T, int n, void* out, int ldo,
                      float* lse2, float* cls_ws, long cls_ws_elems, void* q8out, int ldq8, const float* q8_scale, float* q8_amax,
                      int opts, hipStream_t stream);
int tvts_attn_bwd_q8(int mode, const void* qkv, int ld, int B, int heads, int S, int T, int n, int causal, const void* dO,
              int lddo, const void* O, int ldo, const float* lse2, float* delta, void* dqkv, int lddq, float* cls_acc,
              long cls_acc_elems, void* q8out, int ldq8, const float* q8_scale, float* q8_amax, int opts, hipStream_t stream);

/* the same entry points for head dim 80 (ViT-H/14, 1280 / 16 heads); qkv is [rows, 3*heads*80] */
/* FULL attention over sequences padded to S with the padded keys masked: keys at positions >= kv_len[b] (device int32[B]) get
 * probability 0 -- the attention_mask of the v1 text tower (transformers DistilBERT MultiHeadSelfAttention, reached from
 * v1/model/model_dist_TVTS.py:131-141).  bwd_len = delta + dQ + dK/dV; the dK / dV rows of the padded positions are NOT written
 * (their gradient is zero): zero dqkv first. */
int tvts_attn_fwd_len(const void* qkv, int ld, int B, int heads, int S, const int* kv_len, void* out, int ldo, float* lse2,
                      hipStream_t stream);
int tvts_attn_bwd_len(const void* qkv, int ld, int B, int heads, int S, const int* kv_len, const void* dO, int lddo,
                      const void* O, int ldo, const float* lse2, float* delta, void* dqkv, int lddq, hipStream_t stream);
/* the same pair with DROPOUT on the attention probabilities -- transformers' DistilBERT MultiHeadSelfAttention in training mode
 * (weights = dropout(softmax(scores)), attention_dropout 0.1), which the v1 model runs in every pretraining step
 * (v1/model/model_dist_TVTS.py:33-34 text_model.train(), :131-141).  Counter-based mask: probability (b, h, q, k) is kept iff the
 * upper 32 bits of splitmix64(seed_dev[0] + site + index * 0x9E3779B97F4A7C15) are >= p * 2^32, kept values are scaled by
 * 1 / (1 - p); seed_dev is DEVICE memory (a replayed hipGraph draws new masks when the caller advances it), the backward
 * regenerates the forward's mask from the same (seed, site).  p = 0: the plain pair. */
int tvts_attn_fwd_len_drop(const void* qkv, int ld, int B, int heads, int S, const int* kv_len, void* out, int ldo, float* lse2,
                    float p, const long* seed_dev, long site, hipStream_t stream);
int tvts_attn_bwd_len_drop(const void* qkv, int ld, int B, int heads, int S, const int* kv_len, const void* dO, int lddo,
                    const void* O, int ldo, const float* lse2, float* delta, void* dqkv, int lddq, float p,
                    const long* seed_dev, long site, hipStream_t stream);
/* FULL attention (no mask) whose only QUERIES are the last nq (<= 16) tokens of every sequence, all S tokens keys: the last block
 * of the transcript-sorting head -- SortTransformer.forward_features reads its output at the transcript positions only
 * (v2/model/sort_transformer.py:131-141: x = self.norm(x[:, x_len:])), so the other rows of that block's attention output, MLP and
 * residual are never used by the loss.  out / lse2 / dO / O / delta are indexed by token row (only the query rows are touched);
 * bwd_tail = delta + dQ (query rows) + dK / dV (every row): the caller zeroes the dQ third of the non-query rows of dqkv. */
int tvts_attn_fwd_tail(const void* qkv, int ld, int B, int heads, int S, int nq, void* out, int ldo, float* lse2,
                       hipStream_t stream);
int tvts_attn_bwd_tail(const void* qkv, int ld, int B, int heads, int S, int nq, const void* dO, int lddo, const void* O, int ldo,
                       const float* lse2, float* delta, void* dqkv, int lddq, hipStream_t stream);
int tvts_attn80_fwd_tail(const void* qkv, int ld, int B, int heads, int S, int nq, void* out, int ldo, float* lse2,
                         hipStream_t stream);
int tvts_attn80_bwd_tail(const void* qkv, int ld, int B, int heads, int S, int nq, const void* dO, int lddo, const void* O, int ldo,
                         const float* lse2, float* delta, void* dqkv, int lddq, hipStream_t stream);
/* ONE query per sequence, at token qpos[b] (device int32[B]), that sees the keys 0 .. qpos[b]: the last block of the CLIP text tower,
 * whose output the model reads at the EOT token only (v2/CLIP/clip/model.py:343-354).  Conventions of the tail form; the dK / dV
 * rows behind the query are not written (zero gradient): zero dqkv first. */
int tvts_attn_fwd_rowq(const void* qkv, int ld, int B, int heads, int S, const int* qpos, void* out, int ldo, float* lse2,
                       hipStream_t stream);
int tvts_attn_bwd_rowq(const void* qkv, int ld, int B, int heads, int S, const int* qpos, const void* dO, int lddo, const void* O,
                       int ldo, const float* lse2, float* delta, void* dqkv, int lddq, hipStream_t stream);
int tvts_attn80_fwd_rowq(const void* qkv, int ld, int B, int heads, int S, const int* qpos, void* out, int ldo, float* lse2,
                         hipStream_t stream);
int tvts_attn80_bwd_rowq(const void* qkv, int ld, int B, int heads, int S, const int* qpos, const void* dO, int lddo, const void* O,
                         int ldo, const float* lse2, float* delta, void* dqkv, int lddq, hipStream_t stream);
/* ONE query per sequence at token row 0 over the keys 0 .. nk - 1: nk = S, or with kv_len (device int32[B], optional)
 * nk = clamp(kv_len[b], 1, S), the clamp of tvts_attn_fwd_len.  Forward-only: it writes row b * S of out (and of lse2, if given) and
 * nothing else.  Two sites: the last block of the v1 ViT in the forward-only encoder, which the model reads at the normed CLS token
 * (v1/downstream/video_encoder_zero.py:198-199 `self.norm(x)[:, 0]`), and the last DistilBERT block, whose only consumer is the [CLS]
 * row (v1/model/model_dist_TVTS.py:131-141).  tvts_attn_fwd_len itself takes lse2 == NULL as well (the forward-only DistilBERT
 * blocks in front of the last), with the output bits of the call with lse2. */
int tvts_attn_fwd_first(const void* qkv, int ld, int B, int heads, int S, const int* kv_len, void* out, int ldo, float* lse2,
                        hipStream_t stream);
int tvts_attn80_fwd_first(const void* qkv, int ld, int B, int heads, int S, const int* kv_len, void* out, int ldo, float* lse2,
                          hipStream_t stream);
/* Causal self-attention inside each sequence of a PACKED batch (seq_start as for tvts_text_embed_packed), head dim 64, forward-only
 * (no log-sum-exp): qkv bf16 [M, 3 * heads * 64] -> out bf16 [M, heads * 64]; ld, ldo multiples of 8.  Every length 1 .. 80 in any
 * mixture and order (the CLIP context is 77, CLIP/clip/model.py:330-336); max_len >= the longest sequence selects the tile classes that
 * are launched (lengths 1-16, 17-32, 33-48, 49-80), max_len > 80 returns -22 and a longer sequence is left unwritten.  A wave owns a
 * (sequence, head) group: neighbouring sequences of similar length (a length-sorted packing) keep the waves of a block together.
 * _last: ONE query per sequence at its last row (the EOT token of a packed caption, CLIP/clip/model.py:343-354) over all its keys --
 * the packed counterpart of tvts_attn_fwd_rowq; it writes the rows seq_start[i + 1] - 1 of out and no other. */
int tvts_attn_fwd_packed(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len, void* out, int ldo,
                         hipStream_t stream);
int tvts_attn_fwd_packed_last(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len, void* out, int ldo,
                              hipStream_t stream);
/* Training on packed captions.  _lse: the two entries above (same kernels, the same bits in out) that also store the log2-domain
 * log-sum-exp lse2[row * heads + h] of every packed row they compute (every row of a valid sequence; the N last rows for _last) --
 * layout and units of tvts_attn_fwd / tvts_attn_delta for a [rows = M, heads] problem.
 * tvts_attn_bwd_packed: delta[row * heads + h] = rowsum(dO o O), P = exp2(s * scale2 - lse2), dS = P o (dP - delta), and dQ | dK | dV
 * into the three thirds of dqkv bf16 [M, 3 * heads * 64].  A wave owns a (sequence, head) group (the forward's tile classes and
 * guard) and writes all its rows in all three thirds: no atomics, no prior zeroing, run-to-run the same bits; a sequence with a
 * malformed descriptor is skipped whole (nothing read or written).  _last: backward of the one-query form -- dQ at each sequence's
 * last row, dK / dV at every row, and the dQ third of the other rows of a valid sequence ZEROED BY THE KERNEL; dO, O, lse2 are read
 * and delta is written at the last rows only.  -22: as the forward, or dO / O / lse2 / delta / dqkv NULL, lddo or lddq no multiple of 8. */
int tvts_attn_fwd_packed_lse(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len, void* out, int ldo,
                             float* lse2, hipStream_t stream);
int tvts_attn_fwd_packed_last_lse(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len, void* out,
                                  int ldo, float* lse2, hipStream_t stream);
int tvts_attn_bwd_packed(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len, const void* dO, int lddo,
                         const void* O, int ldo, const float* lse2, float* delta, void* dqkv, int lddq, hipStream_t stream);
int tvts_attn_bwd_packed_last(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len, const void* dO,
                              int lddo, const void* O, int ldo, const float* lse2, float* delta, void* dqkv, int lddq,
                              hipStream_t stream);
/* BIDIRECTIONAL self-attention inside each sequence of a packed batch, with dropout on the probabilities: the DistilBERT tower of v1
 * (v1/model/model_dist_TVTS.py:34,131-141; transformers MultiHeadSelfAttention: weights = dropout(softmax(scores))) over
 * M = sum(len_i) rows instead of N * L.  The kernels, ownership, tile classes, descriptor guard and limits of tvts_attn_fwd_packed /
 * tvts_attn_bwd_packed; every key tile of the sequence is multiplied and only the keys at or behind the sequence end are masked.
 * lse2 (nullable): the layout of tvts_attn_fwd_packed_lse.  Mask rule: probability (sequence i, head h, query q, key k) takes the index
 * ((i * heads + h) * L_pad + q) * L_pad + k of tvts_attn_fwd_len_drop on [N, L_pad] padded captions -- same generator, same
 * (seed_dev, site), so the packed call draws the padded call's mask; the row sum is of the undropped probabilities.  p == 0 runs
 * kernels without any generator work (seed_dev may then be NULL).  The backward regenerates the mask; one wave writes all rows of
 * its group in all three thirds of dqkv: no atomics, no prior zeroing, run-to-run the same bits.
 * _first: ONE query per sequence at its FIRST row ([CLS]) over all its keys, no dropout (the forward-only last block); it writes the
 * rows seq_start[i] of out and no other.
 * -22: as the causal entries (NULL, strides, max_len > 80), or L_pad < max_len, p outside [0, 1), p > 0 with seed_dev NULL. */
int tvts_attn_fwd_packed_bidir(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len, void* out, int ldo,
                               float* lse2, float p, const long* seed_dev, long site, int L_pad, hipStream_t stream);
int tvts_attn_bwd_packed_bidir(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len, const void* dO,
                               int lddo, const void* O, int ldo, const float* lse2, float* delta, void* dqkv, int lddq, float p,
                               const long* seed_dev, long site, int L_pad, hipStream_t stream);
int tvts_attn_fwd_packed_first(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len, void* out, int ldo,
                               hipStream_t stream);
int tvts_attn80_fwd_len(const void* qkv, int ld, int B, int heads, int S, const int* kv_len, void* out, int ldo, float* lse2,
                        hipStream_t stream);
int tvts_attn80_bwd_len(const void* qkv, int ld, int B, int heads, int S, const int* kv_len, const void* dO, int lddo,
                        const void* O, int ldo, const float* lse2, float* delta, void* dqkv, int lddq, hipStream_t stream);
/* the same pair with DROPOUT on the attention probabilities -- transformers' DistilBERT MultiHeadSelfAttention in training mode
 * (weights = dropout(softmax(scores)), attention_dropout 0.1), which the v1 model runs in every pretraining step
 * (v1/model/model_dist_TVTS.py:33-34 text_model.train(), :131-141).  Counter-based mask: probability (b, h, q, k) is kept iff the
 * upper 32 bits of splitmix64(seed_dev[0] + site + index * 0x9E3779B97F4A7C15) are >= p * 2^32, kept values are scaled by
 * 1 / (1 - p); seed_dev is DEVICE memory (a replayed hipGraph draws new masks when the caller advances it), the backward
 * regenerates the forward's mask from the same (seed, site).  p = 0: the plain pair. */
int tvts_attn80_fwd_len_drop(const void* qkv, int ld, int B, int heads, int S, const int* kv_len, void* out, int ldo, float* lse2,
                    float p, const long* seed_dev, long site, hipStream_t stream);
int tvts_attn80_bwd_len_drop(const void* qkv, int ld, int B, int heads, int S, const int* kv_len, const void* dO, int lddo,
                    const void* O, int ldo, const float* lse2, float* delta, void* dqkv, int lddq, float p,
                    const long* seed_dev, long site, hipStream_t stream);
int tvts_attn80_fwd(int mode, const void* qkv, int ld, int B, int heads, int S, int T, int n, int causal, void* out, int ldo,
                  float* lse2, int opts, hipStream_t stream);
int tvts_attn80_delta(const void* dO, int lddo, const void* O, int ldo, int rows, int heads, float* delta,
                    hipStream_t stream);
int tvts_attn80_bwd_dq(int mode, const void* qkv, int ld, int B, int heads, int S, int T, int n, int causal, const void* dO,
                     int lddo, const float* lse2, const float* delta, void* dqkv, int lddq, int opts, hipStream_t stream);
int tvts_attn80_bwd_dkv(int mode, const void* qkv, int ld, int B, int heads, int S, int T, int n, int causal, const void* dO,
                      int lddo, const float* lse2, const float* delta, void* dqkv, int lddq, float* cls_acc, int opts,
                      hipStream_t stream);
int tvts_attn80_cls_finalize(const float* cls_acc, int B, int heads, int S, void* dqkv, int lddq, hipStream_t stream);
/* whole backward of one attention site (D = rowsum(dO*O), dQ, dK, dV, CLS query + CLS key/value reduction of the divided
 * geometries) = the autograd of VarAttention.forward video_encoder_ViT_B_16.py:38-76; delta [rows, heads] and
 * cls_acc (cls_acc_elems fp32 elements) are scratch.  SPACE groups of <= 112 tokens run as ONE fused launch.  cls_acc holds the
 * CLS token's dK / dV / dQ shares: with >= B * heads * max(T, ceil(n / 28)) * 3 * dh elements every block of the fused kernels
 * stores its share and they are added in a fixed order (run-to-run reproducible); with B * heads * 3 * dh elements (the
 * minimum) the shares are accumulated with fp32 atomics. */
int tvts_attn80_bwd(int mode, const void* qkv, int ld, int B, int heads, int S, int T, int n, int causal, const void* dO,
              int lddo, const void* O, int ldo, const float* lse2, float* delta, void* dqkv, int lddq, float* cls_acc,
              long cls_acc_elems, int opts, hipStream_t stream);
/* forward of one divided-attention site including the CLS row (VarAttention.forward video_encoder_ViT_B_16.py:38-76);
 * cls_ws: fp32 scratch of >= B * heads * max(T, ceil(n / 28)) * (dh + 2) elements (partial softmax states of the CLS query) */
int tvts_attn80_fwd_divided(int mode, const void* qkv, int ld, int B, int heads, int S, int T, int n, void* out, int ldo,
                      float* lse2, float* cls_ws, long cls_ws_elems, int opts, hipStream_t stream);
/* the two site entry points with the per-tensor e4m3 copy of their result written by the kernels themselves (BASELINE config 5: the
 * attention output feeds the projection's forward and weight-gradient GEMMs, dqkv the qkv projection's input- and weight-gradient
 * GEMMs): q8out[r, c] = e4m3(result[r, c] / q8_scale[0]) with the result's leading dimension (ldq8 == ldo resp. lddq, in bytes),
 * q8_amax = max(q8_amax, max |result|).  Fused geometries only (SPACE n + 1 <= 112, TIME T + 1 <= 32), -22 otherwise. */
int tvts_attn80_fwd_divided_q8(int mode, const void* qkv, int ld, int B, int heads, int S, int T, int n, void* out, int ldo,
                      float* lse2, float* cls_ws, long cls_ws_elems, void* q8out, int ldq8, const float* q8_scale, float* q8_amax,
                      int opts, hipStream_t stream);
int tvts_attn80_bwd_q8(int mode, const void* qkv, int ld, int B, int heads, int S, int T, int n, int causal, const void* dO,
              int lddo, const void* O, int ldo, const float* lse2, float* delta, void* dqkv, int lddq, float* cls_acc,
              long cls_acc_elems, void* q8out, int ldq8, const float* q8_scale, float* q8_amax, int opts, hipStream_t stream);

/* ---- token assembly (embed.hip): video_encoder_ViT_B_16.py:176-216; model_dist..B_16.py:69-76,98-100;
 *      sort_transformer.py:124-128 */
int tvts_patch_gather(const float* video, const int* keep, int B, int T, int n, int img, int patch, void* out, int ldo,
                      hipStream_t stream);
/* uint8 H x W x 3 frames (resized on the host): crop + ClipToTensor + Normalize (video_transforms/video_transform.py:24-75,
 * functional.py:81-97; base_dataset.py:125-127) fused into the tube-mask gather; mean3 / std3 are HOST arrays, crop is a
 * device [B,2] (top, left) or NULL for the centre crop */
int tvts_patch_gather_u8(const unsigned char* frames, int H0, int W0, const int* crop, const int* keep, int B, int T, int n,
                         int img, int patch, const float* mean3, const float* std3, void* out, int ldo, hipStream_t stream);
/* the same with the transform chain's Resize in front (video_transforms/videoaug.py:12,21 -> video_transform.py:171-188 ->
 * functional.py:47-64: PIL nearest-neighbour to (H0, W0)): frames are the decoder's Hs x Ws pictures, ytab[H0] / xtab[W0]
 * (device int32) hold Pillow's source index of every resized row / column (tvts_amd/data_loader/transforms.py) */
int tvts_patch_gather_u8_resized(const unsigned char* frames, int Hs, int Ws, const int* ytab, const int* xtab, int H0, int W0,
                                 const int* crop, const int* keep, int B, int T, int n, int img, int patch, const float* mean3,
                                 const float* std3, void* out, int ldo, hipStream_t stream);
/* the RAGGED form: the clips of one batch differ in source size, crop and length, as the reference's loaders hand them over -- every
 * clip is resized on its own (v2/video_transforms/videoaug.py:12,21 -> functional.py:47-78) and a clip of fewer than T frames is
 * zero-padded BEHIND Normalize (v2/base/base_dataset.py:116-130: final = zeros; final[:n] = imgs; under "loading": "lax" a failed
 * decode is one black input_res x input_res frame followed by zero frames).
 *   src     one packed byte buffer; clip b is uint8 [frames_b, Hs_b, Ws_b, 3] contiguous at byte offset desc[b][0] (64-bit, ANY
 *           alignment: byte loads only)
 *   desc    int64 [B, 8] in DEVICE memory = (offset, Hs, Ws, top, left, ytab, xtab, frames): (top, left) the crop in RESIZED
 *           coordinates, always explicit (the centre crop is the host's centre_crop_offset); ytab / xtab the int32-element offsets in
 *           `tables` of the clip's row (Hs -> new_h) and column (Ws -> new_w) tables; 1 <= frames <= T
 *   tables  int32 in DEVICE memory, one table per distinct (n_in, n_out) of the batch, shared by the clips that use it:
 *           (n_in, n_out) | index[n_out] -- Pillow's nearest-neighbour source index of every resized row / column
 *           (tvts_amd/data_loader/transforms.py pil_nearest_table); an axis that is not resized has the identity table
 *   out     the rows, columns and padding of tvts_patch_gather_u8: row (b, f, i), columns (ch, py, px), columns 3 * patch^2 .. ldo zero
 * Rows of a frame f >= frames_b are +0 in all ldo columns; for f < frames_b the value is bf16((u / 255.0f - mean) / std) with the
 * operations and order of tvts_patch_gather_u8, the bytes of tvts_patch_gather_u8_resized run on that clip alone.
 * Returns -22 for a NULL src / desc / tables / keep / out / mean3 / std3; B, T, n, patch or img <= 0; img % patch; ldo % 8;
 * ldo < 3 * patch^2.  desc and tables are DEVICE data and are not checked: tvts_amd.hip.check_gather_plan does (every clip inside
 * src, the tables those of its sizes, 0 <= top <= new_h - img, 0 <= left <= new_w - img, 1 <= frames <= T). */
int tvts_patch_gather_u8_ragged(const unsigned char* src, const long* desc, const int* tables, const int* keep, int B, int T, int n,
                                int img, int patch, const float* mean3, const float* std3, void* out, int ldo, hipStream_t stream);
/* tube mask drawn on the device (replaces the per-sample np.random.shuffle(arange(ppf))[:n_keep] of the dataset worker,
 * v2/data_loader/YTTemporal_dataset.py:207-213): keep[b, :] = the n_keep patch indices with the smallest counter-based
 * random keys of sample number first_sample + b -- an unsorted prefix of a uniformly random permutation, shared by all
 * frames of the clip; ppf <= 1024; seed / first_sample are taken as unsigned 64-bit values */
int tvts_tube_mask(long seed, long first_sample, int B, int ppf, int n_keep, int* keep, hipStream_t stream);
/* keep_per_frame 0: keep[B, n], one tube mask for all frames of a clip (v2); 1: keep[B, T, n], one per frame / tubelet (v1) */
int tvts_vit_assemble(const float* patch, int ldp, const float* cls, const float* pos, const float* temporal,
                      const int* keep, int keep_per_frame, int B, int T, int n, int W, float* tok, int ldt, hipStream_t stream);
/* workspace (optional, fp32 scratch): with >= B * ceil(n / 14) * T * W + B * W elements (tube masks) the temporal-embedding and
 * class-embedding sums are ordered per-block partials; with B * n * W more and n_pos > 0 (the rows of dpos behind the class row:
 * the patches per frame) the positional-embedding rows are gathered in clip order too -- every sum run-to-run reproducible.
 * One keep list per frame / tubelet (v1): B * T * W + B * W + B * T * n * W elements for the same.  Without the room (or
 * n_pos = 0) they are a scatter of fp32 atomics. */
int tvts_vit_assemble_bwd(const float* dtok, int ldt, const int* keep, int keep_per_frame, int B, int T, int n, int W,
                          void* dpatch, int ldp, float* dcls, float* dpos, int n_pos, float* dtemporal, float* workspace,
                          long workspace_elems, hipStream_t stream);
/* ---- v1 (TVTS) Conv3d tubelet embedding as im2col over the kept patches of every tube (v1/model/video_encoder.py:78-99,199-206):
 * keep int32 [B, tubes, n] -> bf16 rows [B * tubes * n, 3 * tubelet * patch^2] in the Conv3d weight's (c, t, py, px) column order.
 * The seven entry points below are ONE kernel frame (embed.hip: tube_gather_kernel -- row and column decode, keep lookup, the
 * optional mix, the bf16 rounding and the store) over four source policies (fp32 clip, uint8 crop, uint8 view, uint8 augmentation), so
 * every "same bits as" statement below holds by construction: the forms named share the frame, and the uint8 forms share one
 * normalise expression, bf16((u / 255.0f - mean) / std) with the operations and their order those of tvts_patch_gather_u8 -- the
 * bytes of the fp32 forms on host-normalised frames.
 * All seven return -22 for: a NULL source / keep / out (and mean3 / std3, HOST arrays, in the uint8 forms; and the form's table);
 * B, tubes, tubelet, n, patch or img <= 0; img % patch; patch % 8; ldo % 8 or ldo < 3 * tubelet * patch^2 (a wider leading dimension
 * is left untouched); out not 16-byte aligned; an fp32 video not 16-byte aligned; H0 < img or W0 < img where a crop of img x img is
 * cut from the frames (all uint8 forms but _aug).  crop and the tables are DEVICE data and are not checked: the caller keeps them in
 * range (tvts_amd.hip.mix_table / aug_table / view_table do); a crop outside the frame reads outside the frames.
 * video fp32 [B, tubes * tubelet, 3, img, img]: */
int tvts_patch_gather_tube(const float* video, const int* keep, int B, int tubes, int tubelet, int n, int img, int patch,
                           void* out, int ldo, hipStream_t stream);
/* CHANNEL-MAJOR fp32 clips [B, 3, tubes * tubelet, img, img], the layout the v1 downstream classes take
 * (v1/downstream/video_encoder_zero.py:91-96,177: forward_features hands x to the Conv3d as it comes): the same frame and load, so
 * the bytes of tvts_patch_gather_tube on the permuted clip */
int tvts_patch_gather_tube_cm(const float* video, const int* keep, int B, int tubes, int tubelet, int n, int img, int patch,
                              void* out, int ldo, hipStream_t stream);
/* uint8 frames [B, tubes * tubelet, H0, W0, 3]: crop (device [B,2] (top, left), 0 <= top <= H0 - img and 0 <= left <= W0 - img, or
 * NULL for the centre crop with the round-half-to-even offsets of tvts_patch_gather_u8) + ClipToTensor + Normalize of the v1
 * downstream pipeline (v1/downstream/ssv2.py:61-63) fused into the gather */
int tvts_patch_gather_tube_u8(const unsigned char* frames, int H0, int W0, const int* crop, const int* keep, int B, int tubes,
                              int tubelet, int n, int img, int patch, const float* mean3, const float* std3, void* out, int ldo,
                              hipStream_t stream);
/* Mixup / CutMix of the v1 fine-tuning recipe (v1/downstream/mixup.py:152-200 `_mix_elem` / `_mix_pair` / `_mix_batch`, applied as
 * `samples, targets = mixup_fn(samples, targets)` at v1/downstream/engine_for_finetuning.py:58-59) applied by the frame per element in
 * front of the bf16 rounding, here over tvts_patch_gather_tube_cm's source.  The step's draw is a per-sample table in DEVICE memory:
 * mix_i int32 [B, 6] = (partner, mode, yl, yh, xl, xh), mode 0 none / 1 mixup / 2 cutmix / 3 pair-mode cutmix (below), the box
 * half-open in image coordinates behind the crop, 0 <= lo <= hi <= img; mix_f fp32 [B, 2] = (lam, one_minus_lam), both rounded by the host.
 * mode 0: the own value, bits untouched; mode 1: fadd_rn(fmul_rn(own, lam), fmul_rn(partner, one_minus_lam)) (two rounded
 * products, then the sum: mixup.py:198-199, never an FMA); mode 2: the partner's value inside the box of every channel and frame
 * (mixup.py:163,196), the own value outside; mode 3: what `_mix_pair` does to a 5-D clip batch -- `x[i][:, yl:yh, xl:xh]`
 * (mixup.py:180-181) slices a [C, T, H, W] clip by (frame, row): the partner's value in the frames [yl, yh) (cut at T) and the rows
 * [xl, xh) of every channel, whole rows; the own value elsewhere.  One table serves the reference's batch / pair / elem modes.
 * A partner outside [0, B) leaves that sample's rows unwritten. */
int tvts_patch_gather_tube_cm_mix(const float* video, const int* keep, const int* mix_i, const float* mix_f, int B, int tubes,
                                  int tubelet, int n, int img, int patch, void* out, int ldo, hipStream_t stream);
/* the same mix over tvts_patch_gather_tube_u8's source: each of the two samples is cropped with ITS OWN crop offset and normalised,
 * the normalised fp32 values are mixed and rounded to bf16 -- the bytes of tvts_patch_gather_tube_cm_mix on host-cropped,
 * host-normalised frames */
int tvts_patch_gather_tube_u8_mix(const unsigned char* frames, int H0, int W0, const int* crop, const int* keep, const int* mix_i,
                                  const float* mix_f, int B, int tubes, int tubelet, int n, int img, int patch, const float* mean3,
                                  const float* std3, void* out, int ldo, hipStream_t stream);
/* The per-sample augmentation of the v1 fine-tuning recipe behind RandAugment (v1/downstream/ssv2.py:186-227) as the frame's source:
 * Normalize, `random_resized_crop` (v1/downstream/video_transforms.py:499-573: `_get_param_spatial_crop`, then torch's
 * bilinear `interpolate(..., align_corners=False)` of the crop to img x img), `horizontal_flip` (video_transforms.py:156-177),
 * `RandomErasing._erase_cube` (v1/downstream/random_erasing.py:109-149), then the frame's mix (mix_i / mix_f both given or both
 * NULL).  frames uint8 [Bs, T, H0, W0, 3], Bs >= 1; H0, W0 >= 1 (source frames may be smaller than img).  The draw is a per-sample
 * table in DEVICE memory:
 *   aug_i int32 [B, 16] = (src, top, left, h, w, flip, emode, etop, eleft, eh, ew, key_lo, key_hi, 0, 0, 0)
 * src: the source clip in [0, Bs) -- several samples may name one clip (the two views of `--num_sample 2`,
 * v1/downstream/utils.py `multiple_samples_collate`); [top, top + h) x [left, left + w): the crop in the source frame, 1 <= h <= H0,
 * 1 <= w <= W0; flip 0 / 1: the resized picture mirrored in x; emode 0 none / 1 const (zeros) / 2 rand (one normal per frame and
 * channel) / 3 pixel (one normal per frame, channel and pixel); [etop, etop + eh) x [eleft, eleft + ew): the erase box in OUTPUT
 * coordinates, the same in every frame; key = key_lo | key_hi << 32: the sample's noise key.
 * Output element (b, c, f, y, x), in this order:
 *   taps   sy = (float)h / (float)img, s = max(sy * (y + 0.5f) - 0.5f, 0), y0 = (int)s, y1 = min(y0 + 1, h - 1) (the crop's edge, not
 *          the frame's), ly = s - y0; the same in x with w, x replaced by img - 1 - x first under flip.  fp32, every operation rounded.
 *   values the four taps of frame src * T + f at (top + y., left + x.), each normalised by the shared expression
 *   blend  (1 - ly) * ((1 - lx) * a + lx * b) + ly * ((1 - lx) * c + lx * d), every product and sum rounded to fp32 (no FMA).  With
 *          h == w == img, flip == 0, emode == 0 every l is 0 and the bits are tvts_patch_gather_tube_u8's with crop = (top, left).
 *   erase  inside the box: const 0.0f; pixel z(key, ((f * 3 + c) * img + y) * img + x); rand z(key + 0xD1B54A32D192ED03, f * 3 + c).  The
 *          index is in output coordinates: a pixel's noise depends on neither keep, the patch size nor the thread that holds it.
 *   mix    the frame's mix over this value and the partner's, the partner taken through ITS OWN crop, flip and erase; then ONE
 *          rounding to bf16.
 * z(key, idx): r = mix(key + idx * 0x9E3779B97F4A7C15) with the splitmix64 finaliser of the dropout masks above; u1 = ((r >> 32) + 1)
 * * 2^-32 in (0, 1], u2 = (r & 0xffffffff) * 2^-32, z = sqrtf(-2 logf(u1)) * cosf(2 pi u2), the accurate library functions, ln u1
 * taken as log1pf(u1 - 1) where u1 is within 2^-8 of 1 (an fp32 u1 has lost ln u1 there): within 2e-5 of the rule evaluated in
 * float64, which is its definition.  The reference draws this noise from
 * torch's CPU generator (random_erasing.py:11-24 `_get_pixels`); that stream is not reproduced.
 * A src outside [0, Bs) -- the sample's own or, under a mix, its partner's -- leaves that sample's rows unwritten and reads nothing. */
int tvts_patch_gather_tube_u8_aug(const unsigned char* frames, int Bs, int H0, int W0, const int* keep, const int* aug_i,
                                  const int* mix_i, const float* mix_f, int B, int tubes, int tubelet, int n, int img, int patch,
                                  const float* mean3, const float* std3, void* out, int ldo, hipStream_t stream);
/* The test views of v1/downstream/ssv2.py:132-164 (mode 'test') as the frame's source: every sample is a strided run of frames of
 * a source clip, cropped at an offset -- `buffer[temporal_start::2, spatial_start:spatial_start + short_side_size]` -- so the
 * test_num_segment x test_num_crop views of a video read ONE uploaded clip.  frames uint8 [Bs, Tsrc, H0, W0, 3], Bs, Tsrc >= 1; the
 * views are a per-sample table in DEVICE memory:
 *   view_i int32 [B, 8] = (src, t0, tstep, top, left, 0, 0, 0)
 * frame f (0 <= f < tubes * tubelet) of sample b is frame t0 + f * tstep < Tsrc of source clip src, cropped to [top, top + img) x
 * [left, left + img); several samples may name one clip.  Only the source address differs from tvts_patch_gather_tube_u8: the bytes
 * equal its bytes on the host-sliced clip frames[src, t0::tstep][:T, top:top + img, left:left + img].  No resampling: the short-side
 * Resize in front of the slicing (ssv2.py:147) is the host's, beside decoding.  A src outside [0, Bs) leaves that sample's rows
 * unwritten and reads nothing. */
int tvts_patch_gather_tube_u8_view(const unsigned char* frames, int Bs, int Tsrc, int H0, int W0, const int* view_i, const int* keep,
                                   int B, int tubes, int tubelet, int n, int img, int patch, const float* mean3, const float* std3,
                                   void* out, int ldo, hipStream_t stream);
/* ---- The Resize and crop of the v1 PRETRAINING transform on uint8 frames at source size, in front of tvts_patch_gather_tube_u8
 * (v1/video_transforms/videoaug.py:8-22: TensorToNumpy -> Resize(int(crop * 1.2)) -> RandomCrop | CenterCrop -> ClipToTensor ->
 * Normalize).  TensorToNumpy makes PIL images and v1/video_transforms/functional.py:56-59 maps every interpolation but 'bilinear' --
 * the default 'nearest' included -- to PIL.Image.BILINEAR, so the Resize is Pillow's 8-bit bilinear resample (Resample.c,
 * PRECISION_BITS = 22): two passes with fixed-point taps and a support that grows with the downscale.  It is integer arithmetic; the
 * bytes written are Pillow's, `resized[top:top + img, left:left + img]` of every frame, and only that window is computed.
 *   src     one packed byte buffer of source clips; clip b is uint8 [T, Hs_b, Ws_b, 3] contiguous at byte offset desc[b][0] (64-bit, any
 *           alignment); the clips of one batch may differ in Hs_b x Ws_b
 *   desc    int64 [B, 8] in DEVICE memory = (offset, Hs, Ws, top, left, ytab, xtab, 0): (top, left) the crop in RESIZED coordinates,
 *           ytab / xtab the int32-element offsets in `tables` of the clip's row (Hs -> new_h) and column (Ws -> new_w) tables
 *   tables  int32 in DEVICE memory, one table per distinct (n_in, n_out) of the batch, shared by the clips that use it:
 *           (n_in, n_out, ksize, 0) | first[n_out] | count[n_out] | taps[n_out][ksize] -- output index i reads the source indices
 *           first[i] .. first[i] + count[i] - 1 with the int32 taps taps[i][0 .. count[i]) (tvts_amd/data_loader/transforms.py
 *           pil_bilinear_coeffs: Pillow's precompute_coeffs + normalize_coeffs_8bpc), 1 <= count[i] <= ksize
 *   out     uint8 [B, T, img, img, 3], pixel rows ldo >= 3 * img bytes apart (3 * img: the contiguous clips the gather takes)
 * One pass: acc = 2^21 + sum_j px[first + j] * taps[j] (int32: the taps are >= 0 and sum to 2^22 +- count), byte = clip8(acc >> 22).
 * The horizontal pass runs first, over the source rows the vertical taps of the window read; the vertical pass reads its ROUNDED
 * uint8 result (the rounding between the passes is part of Pillow's result).  An axis whose size does not change has identity taps.
 * Intermediate storage: a buffer of the CALLER (nothing is allocated here), tmp uint8 [B, T, tmp_rows, img, 3] -- tmp_bytes >=
 * B * T * tmp_rows * img * 3, tmp_rows >= the largest row span of a window in the batch, first[top + img - 1] + count[top + img - 1] -
 * first[top] of a clip's row table (tvts_amd.hip.check_resize_plan returns it).  A window that would need more rows is cut at
 * tmp_rows (its lower rows are wrong, nothing is written outside tmp or out).
 * Returns -22 for a NULL src / desc / tables / tmp / out; B, T, img or tmp_rows <= 0 (B, T > 65535; img, tmp_rows > 32768); ldo < 3 * img;
 * tmp_bytes below the rule.  desc and tables are DEVICE data and are not checked: tvts_amd.hip.check_resize_plan does (0 <= top <=
 * new_h - img, 0 <= left <= new_w - img, every clip inside src, the tables those of its sizes). */
int tvts_resize_crop_u8(const unsigned char* src, const long* desc, const int* tables, int B, int T, int img, int tmp_rows,
                        unsigned char* tmp, long tmp_bytes, unsigned char* out, int ldo, hipStream_t stream);
/* ---- RandAugment of the v1 fine-tuning recipe (v1/downstream/rand_augment.py applied at v1/downstream/ssv2.py:174-184, --aa
 * rand-m7-n4-mstd0.5-inc1) on uint8 frames at source size, in front of the augmentation gather above, with the bytes PIL gives.
 * work uint8 [Bs + 2 * B, T, H0, W0, 3]: the Bs uploaded source clips, then two regions of B views each.  B = Bs * num_sample views;
 * view b belongs to source clip b / num_sample.  The draw is a per-view table of L <= 8 layers in DEVICE memory, the active ops of a
 * view compacted to the front of its row (tvts_amd.hip.check_randaug_plan checks it; here it is unchecked device data):
 *   ra_i int32   [B, L, 4] = (op, resample, iarg, 0)           ra_d float64 [B, L, 8] = (a, b, c, d, e, f, factor, 0)
 * op 0 none, 1 AutoContrast, 2 Equalize, 3 Invert, 4 Solarize(iarg = threshold, 0..256), 5 SolarizeAdd(iarg = add), 6 Posterize(iarg
 * = bits kept, 0..7), 7 Color, 8 Contrast, 9 Brightness, 10 Sharpness (7-10: factor), 11 Affine (a..f, resample 2 bilinear / 3
 * bicubic -- PIL's constants: ShearX / ShearY / TranslateXRel / TranslateYRel / Rotate all arrive as the six coefficients PIL's
 * Image.transform hands its C code).  One call handles ONE layer: layer j reads view b from clip b / num_sample (j = 0) or from
 * clip Bs + ((j - 1) & 1) * B + b, and writes clip Bs + (j & 1) * B + b -- only for a view whose op in layer j is 1..11.  A view with
 * k active ops therefore ends in its source clip (k = 0), the first region (k odd) or the second (k even, k > 0); nothing is copied.
 * Arithmetic (no product-sum of it is contracted into an FMA), c = channel:
 *   3-6    a 256-entry table: 255 - i; i < thr ? i : 255 - i; i < 128 ? min(255, i + add) : i; i & ~(2^(8 - bits) - 1)
 *   1      per frame and channel, lo / hi the first / last nonzero histogram bin: hi <= lo the identity, else scale = 255.0 / (hi -
 *          lo), off = -lo * scale, table[i] = clamp((int)(i * scale + off), 0, 255), in double
 *   2      per frame and channel: one nonzero bin or fewer the identity; step = (N - the last nonzero count) / 255 (integers), 0 the
 *          identity; n = step / 2, then for i = 0 .. 255: table[i] = min(n / step, 255), n += h[i]
 *   7-10   t = (float)d + factor * ((float)i - (float)d) in float, the result (int)t for 0 <= factor <= 1, else t clamped to [0, 255]
 *          first; d = 0 (Brightness); L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 (Color); the constant (int)(mean(L) + 0.5),
 *          the mean the exact sum of the L histogram over the pixel count in double (Contrast); the 3 x 3 filter (1 1 1 / 1 5 1 /
 *          1 1 1) / 13 in float -- 0.5f, then += the three products of the row below, of the row itself, of the row above, each
 *          summed left to right; clamped and truncated; the frame's one-pixel border unfiltered (Sharpness)
 *   11     xin = a * (x + 0.5) + b * (y + 0.5) + c, yin the same with d, e, f, in double; outside [0, W0) x [0, H0): 128; else both
 *          - 0.5, floor, fractions dx, dy, tap coordinates clamped to the frame; bilinear v1 = p00 + (p01 - p00) * dx, v2 the same
 *          one row down, (int)(v1 + (v2 - v1) * dy); bicubic 4 x 4 taps, rows first, each p1 + d * (p2 + d * (p3 + d * p4)) with
 *          p1 = v2, p2 = -v1 + v3, p3 = 2 * (v1 - v2) + v3 - v4, p4 = -v1 + v2 - v3 + v4; 0 for v <= 0, 255 for v >= 255, else (int)v
 * tvts_randaug_hist: hist uint32 [B, T, 4 (R, G, B, L), 256] of the frames layer `layer` reads, for the views whose op there is 1, 2
 * or 8 (the rest stays 0); zeroed on the stream first; integer atomics, so independent of order.  tvts_randaug_apply: hist may be
 * NULL when no view's op in the layer is 1, 2 or 8 (such a view is then left unwritten).
 * Both return -22 for a NULL work / ra_i (/ ra_d; / hist in _hist), Bs, B, num_sample, T <= 0, B != Bs * num_sample, B or T > 65535,
 * H0 < 3 or W0 < 3, L outside [1, 8], layer outside [0, L). */
int tvts_randaug_hist(const unsigned char* work, int Bs, int B, int num_sample, int T, int H0, int W0, int layer, int L,
                      const int* ra_i, unsigned int* hist, hipStream_t stream);
int tvts_randaug_apply(unsigned char* work, int Bs, int B, int num_sample, int T, int H0, int W0, int layer, int L, const int* ra_i,
                       const double* ra_d, const unsigned int* hist, hipStream_t stream);
int tvts_text_embed(const int* ids, int ld_ids, int N, int L, const float* emb, const float* pos, int Wt, float* x, int ldx,
                    hipStream_t stream);
/* ---- PACKED variable-length captions (the forward-only text encoder of the SSv2 multiple-choice models,
 * v2/downstream/zero_ssv2_mc_TVTSv2_ViT_B_16.py:60-88: C x B ragged captions per batch).  One descriptor for every sequence-aware entry
 * point: seq_start, device int32[N + 1], ascending, seq_start[0] = 0, seq_start[N] = M; sequence i owns the token rows
 * seq_start[i] .. seq_start[i + 1] - 1.  A sequence whose descriptor leaves [0, M) is skipped (nothing read or written for it).
 * x[r] = emb[ids[r]] + pos[r - seq_start[i]] for the packed ids int32[M] (one fp32 add per element); rows whose token id is outside
 * [0, vocab) or whose position is >= context are left unwritten. */
int tvts_text_embed_packed(const int* ids, const int* seq_start, int N, int M, const float* emb, const float* pos, int Wt, int vocab,
                           int context, float* x, int ldx, hipStream_t stream);
/* order / seg (optional, device int32): the rows 0 .. N * L - 1 sorted by token id (ties in row order) and the starts of the runs
 * of equal ids in that list (N * L + 1 entries, non-decreasing, padded with N * L) -- with them both embedding gradients are
 * ordered sums (run-to-run reproducible), without them (NULL) a scatter of fp32 atomics like nn.Embedding's backward.  The runs
 * may be listed in any order; runs of more than 64 rows among the FIRST 64 are summed by a block per 64 columns instead of one
 * block (list the long ones first: every caption's start / end token makes a run of N rows) */
int tvts_text_embed_bwd(const float* dx, int ldx, const int* ids, int ld_ids, int N, int L, int Wt, float* demb, float* dpos,
                        const int* order, const int* seg, hipStream_t stream);
/* the same for packed captions (ids int32[M], seq_start int32[N + 1]), ordered sums only: demb[id] += the rows of a run of tok_order /
 * tok_seg (the plan of tvts_text_embed_bwd over the flat ids, M + 1 starts), dpos[l] += the rows pos_order[pos_seg[l] .. pos_seg[l + 1])
 * in that order (rows sorted stably by r - seq_start[seq(r)], context + 1 starts).  An id outside [0, vocab) or a position outside
 * [0, context) adds nothing. */
int tvts_text_embed_bwd_packed(const float* dx, int ldx, const int* ids, const int* seq_start, int N, int M, int Wt, int vocab,
                               int context, float* demb, float* dpos, const int* tok_order, const int* tok_seg, const int* pos_order,
                               const int* pos_seg, hipStream_t stream);
int tvts_text_mean(const float* t, int NT, int B, int E, float* mean, float* before, hipStream_t stream);
int tvts_text_mean_bwd(const float* dmean, int NT, int B, int E, float* dt, hipStream_t stream);
int tvts_sort_assemble(const float* tok, int ldt, int B, int S, int off, int Sv, const float* text, int NT,
                       const float* type, int E, float* xs, int ldx, hipStream_t stream);
/* workspace (optional, >= B * (ceil(S / 32) + 1) * E fp32 elements): the type-embedding gradient as ordered partials (no atomics) */
int tvts_sort_assemble_bwd(const float* dxs, int ldx, int B, int S, int off, int Sv, int NT, const float* dvid, int E,
                           void* dout, int ldo, float* dtype, float* workspace, long workspace_elems, hipStream_t stream);
/* hidden-state dropout of the v1 text tower in training mode (transformers DistilBERT: Embeddings.dropout after the embedding
 * LayerNorm, FFN.dropout after lin2; p = 0.1; v1/model/model_dist_TVTS.py:33-34): out[r, c] = x[r, c] * m / (1 - p) (+ residual[r, c]),
 * m from the same counter-based generator as the attention dropout with index r * cols + c; out (fp32) and / or out_bf16 may be
 * given.  The backward is the same call on the gradient (same seed / site => same mask). */
int tvts_dropout_rows(const float* x, int ldx, int rows, int cols, float p, const long* seed_dev, long site,
                      const float* residual, int ldr, float* out, int ldo, void* out_bf16, int ldob, hipStream_t stream);
/* the same over PACKED captions (x [M, cols], seq_start device int32[N + 1] as for tvts_text_embed_packed): element (r, c) with
 * r = seq_start[i] + t uses the index (i * L_pad + t) * cols + c of its PADDED position, so the call draws the mask tvts_dropout_rows
 * draws on the [N * L_pad, cols] buffer of the padded step (L_pad: that step's L, the longest caption).  The embedding dropout, every
 * FFN.dropout and their backward calls of the v1 step with arch["text_unpadded"].  A row outside every caption or at a position
 * >= L_pad is left unwritten.  -22: x / seq_start / seed_dev NULL, neither output, N, M, cols or L_pad <= 0, p outside [0, 1), a
 * leading dimension below cols. */
int tvts_dropout_rows_packed(const float* x, int ldx, const int* seq_start, int N, int M, int cols, int L_pad, float p,
                             const long* seed_dev, long site, const float* residual, int ldr, float* out, int ldo, void* out_bf16,
                             int ldob, hipStream_t stream);
/* out = relu(x) (dy NULL) or out = dy * (x > 0) (its backward): the nn.ReLU of v1's txt_proj (v1/model/model_dist_TVTS.py:65-68) */
int tvts_relu(const float* x, const float* dy, float* out, long n, hipStream_t stream);
int tvts_rows_gather(const float* src, int ld_src, const int* rows, int R, int W, float* dst, int ld_dst, int scatter_add,
                     hipStream_t stream);
/* rows between a token-row matrix ("full") and a packed [R, W] matrix: the last block of the sort head (sort_transformer.py:131-141:
   the model reads the NT transcript rows) and of the text tower (CLIP/clip/model.py:343-354: the EOT row) run on those R rows only.
   mode 0 gather: packed[r] = full[rows[r]] (source full_f32 if given, else full_bf16; packed_f32 and / or packed_bf16 written);
   mode 1 scatter: full[rows[r]] = packed[r] for every element type given on both sides; mode 2: full_f32[rows[r]] += packed_f32[r] and
   full_bf16[rows[r]] = bf16(sum) when given.  rows must be distinct. */
int tvts_rows_move(int mode, const int* rows, int R, int W, float* full_f32, int ld_full_f32, void* full_bf16, int ld_full_bf16,
                   float* packed_f32, int ld_packed_f32, void* packed_bf16, int ld_packed_bf16, hipStream_t stream);
/* x[r, 0:cols] = 0 of a bf16 matrix (cols, ld multiples of 8): dQ of the rows that are no queries in the used-rows attention backward */
int tvts_zero_cols_bf16(void* x, int ld, long rows, int cols, hipStream_t stream);

/* ---- losses (loss.hip): model_dist..B_16.py:119-127, loss.py:13-25, trainer.py:487-492 */
int tvts_l2norm_rows(const float* x, int R, int E, float eps, float* xn, float* inv, hipStream_t stream);
int tvts_l2norm_rows_bwd(const float* dxn, const float* xn, const float* inv, int R, int E, float* dx, hipStream_t stream);
int tvts_infonce(const float* x, int G, float* lse, float* dx, float* loss, hipStream_t stream);
int tvts_cross_entropy(const float* logits, const int* labels, int R, int C, float scale, float* dlogits, float* loss,
                       hipStream_t stream);
/* SSv2 multiple-choice scoring (v2/downstream/zero_ssv2_mc_TVTSv2_ViT_B_16.py:80-88) in one launch: text fp32 [C, B, E] (option-major,
 * as the _mc models return it), video fp32 [B, E] -> logits[b, c] = 100 <v_b, t_cb> / (|v_b| |t_cb|), fp32 [B, C]; plain norms (no
 * eps clamp), fixed summation order (two runs give the same bits) */
int tvts_mc_logits(const float* text, const float* video, int C, int B, int E, float* logits, hipStream_t stream);
/* validation: rank of the ground truth per query in sims[n_text, n_vid] (text x video);
 * mode 0 = model/metric.py:16-126 t2v_metrics (ranks[n_text], optimistic ties), mode 1 = :129-187 v2t_metrics
 * (ranks[n_vid], averaged ties, closest own caption); valid: optional n_text bytes, 0 = caption missing (query_masks) */
int tvts_retrieval_ranks(const float* sims, long ld, int n_text, int n_vid, int mode, const unsigned char* valid,
                         float* ranks, hipStream_t stream);

/* v1's zero-shot protocol, video-to-video retrieval by label (v1/downstream/run_class_zero.py:344-413): row i of sims[nq, >= N] holds
 * the similarities of query video q0 + i to all N videos, element [i, q0 + i] is read as -1000 (the script's self-mask :385-387; sims
 * is not modified), labels int32[N].  ranks[i] = #{ j : labels[j] != labels[q] and s'[i, j] > best_i } with best_i = max{ s'[i, j] :
 * labels[j] == labels[q] } (self included at -1000): `ranks < k` is the script's hit among the first k of argsort(-scores), k <= 10
 * (:389-404).  Strict > (ties optimistic, as mode 0 above); exact integers; 0 <= q0, q0 + nq <= N, ld >= N, N < 2^24 (the counts are
 * summed in fp32, exact below that; -22 otherwise). */
int tvts_v2v_ranks(const float* sims, long ld, int nq, int q0, int N, const int* labels, float* ranks, hipStream_t stream);

/* ---- optimizer (optim.hip): transformers.AdamW as built at train_dist_TVTSv2_ViT_B_16.py:118-125 */
/* step_dev (optional): the step counter in device memory (hipGraph replay); hyper_dev (optional, needs step_dev): lr[4] | wd[4]
 * in device memory, read instead of the host lr4 / wd4 so that a captured launch follows the LR schedule */
int tvts_adamw_hf(float* p, const float* g, float* m, float* v, void* shadow_bf16, const unsigned char* chunk_group,
                  int nchunks, const float* lr4, const float* wd4, int step, const int* step_dev, const float* hyper_dev,
                  double beta1, double beta2, double eps, float grad_scale, hipStream_t stream);
/* The same rule for the pretraining step with gradient clipping and the overflow guard (StepRunner(clip_grad=, skip_nonfinite=)).
 * The arguments of tvts_adamw_hf plus norm_coef (optional) and skipped (optional); step_dev is written under the guard.
 * g = stored gradient * grad_scale * norm_coef[1], multiplied in that order (two fp32 roundings), norm_coef = what tvts_grad_sumsq left
 * in device memory.  norm_coef null, or a coefficient of exactly 1.0f: the bits of tvts_adamw_hf.  skipped != null: the guard as
 * described above tvts_swap_f32_shadow -- norm_coef[0] finite: step_dev[0] += 1 first, then the unguarded update with that count, bit
 * for bit; not finite: every bit of p, m, v and the shadow is kept, step_dev[0] stays, skipped[0] += 1; `step` is ignored.
 * -22: p, g, m or v null or not 16-byte aligned; chunk_group, lr4 or wd4 null; nchunks <= 0; shadow / skipped not 8-byte aligned,
 * step_dev / norm_coef / hyper_dev not 4; step <= 0 without step_dev; hyper_dev without step_dev; under the guard step_dev or
 * norm_coef null. */
int tvts_adamw_hf_guarded(float* p, const float* g, float* m, float* v, void* shadow_bf16, const unsigned char* chunk_group,
                          int nchunks, const float* lr4, const float* wd4, int step, int* step_dev, const float* hyper_dev,
                          double beta1, double beta2, double eps, float grad_scale, const float* norm_coef, long* skipped,
                          hipStream_t stream);
int tvts_cast_f32_bf16(const float* src, void* dst, long n, hipStream_t stream);
int tvts_cast_bf16_f32(const void* src, float* dst, long n, hipStream_t stream);
int tvts_transpose_bf16_batched(const void* src, void* dst, const void* tiles, int ntiles, hipStream_t stream);
/* H/14 (patch 14, K = 588): video_encoder_ViT_H_14.py:336-337 conv1 weight padded to K = 640 for the MFMA GEMM */
int tvts_pad_rows_bf16(const void* src, int ld_src, void* dst, int ld_dst, int rows, int cols, int cols_pad,
                       hipStream_t stream);
int tvts_add_rows_f32(float* dst, int ld_dst, const float* src, int ld_src, int rows, int cols, hipStream_t stream);
int tvts_probe_tr16(const void* in, void* out, hipStream_t stream);

/* ---- v1 action-recognition fine-tuning (finetune.hip): what v1/downstream/run_class_finetuning.py adds on top of the tower */
/* timm DropPath as v1/downstream/video_encoder.py:65,71-72 uses it, rates video_encoder.py:138: scale[nsites, B] fp32, site 2 l =
 * the attention branch of block l, 2 l + 1 = its MLP branch; sample b of site s is kept iff the upper 32 bits of the counter-based
 * generator at (seed_dev[0] + (site_base + s) * site stride, b) are >= p_sites[s] * 2^32 (mixing: see the kernel comment);
 * scale = keep ? 1 / (1 - p) : 0; p <= 0 gives exactly 1.0f.  p_sites: device fp32 [nsites]. */
int tvts_drop_path_table(const long* seed_dev, long site_base, const float* p_sites, int nsites, int B, float* scale,
                         hipStream_t stream);
/* video_encoder.py:71-72 `x + drop_path(branch(x))`: out[r, :] = residual[r, :] + scale[r / S] * y[r, :] (fp32 y / residual, fp32
 * and / or bf16 out, 16-byte accesses: cols % 4 == 0, strides % 4 == 0).  residual == NULL: the backward, out = scale[r / S] * y.
 * scale 0 copies the residual's bits (exact zeros without one); scale 1 is the plain fp32 add.  rows % S == 0. */
int tvts_drop_path_rows(const float* y, long ldy, long rows, int cols, int S, const float* scale, const float* residual, long ldr,
                        float* out, long ldo, void* out_bf16, long ldob, hipStream_t stream);
/* run_class_finetuning.py:423-427: timm SoftTargetCrossEntropy on soft_targets [B, C] (mean_b sum_c -t log_softmax(x)), or -- labels
 * int32 [B] + smoothing -- LabelSmoothingCrossEntropy ((1 - eps) nll + eps mean_c(-logp); eps = 0: nn.CrossEntropyLoss).  Exactly
 * one of soft_targets / labels.  loss_acc[0] += scale * loss (fixed summation order); dlogits (optional) = scale / B * (softmax *
 * sum_c t - t); hits (optional) = #{b : argmax x == argmax t} (engine_for_finetuning.py:104).  ws: fp32 [2 B] scratch. */
int tvts_soft_ce(const float* logits, long ld, int B, int C, const float* soft_targets, long ldt, const int* labels,
                 float smoothing, float scale, float* loss_acc, float* dlogits, long ldd, int* hits, float* ws, hipStream_t stream);
/* mixup_target (v1/downstream/mixup.py:18-23) over the mix table of tvts_patch_gather_tube_cm_mix: out fp32 [B, C] (ldo >= C, a
 * wider leading dimension is left untouched), t[b, c] = fadd_rn(fmul_rn(y1, lam), fmul_rn(y2, one_minus_lam)) with y1 / y2 the on /
 * off value for labels[b] / labels[partner[b]]; off = smoothing / C and on = 1 - smoothing + off are computed in double and rounded to
 * fp32 as torch.full does.  Mode-0 rows take lam = 1, one_minus_lam = 0 and still run the arithmetic (the reference computes
 * y1 * 1. + y2 * 0.).  labels int32 [B] and the table are DEVICE data and are not checked; a partner outside [0, B) leaves its row
 * unwritten.  The result feeds tvts_soft_ce(soft_targets = ...). */
int tvts_mix_targets(const int* labels, const int* mix_i, const float* mix_f, int B, int C, double smoothing, float* out, long ldo,
                     hipStream_t stream);
/* ---- evaluation of the fine-tuned classifier (v1/downstream/engine_for_finetuning.py:142-285: validation_one_epoch, final_test, merge) */
/* The rank of the label's logit among a row's logits: x fp32 [R, C] (ld >= C), labels int32 [R] -> ranks int32 [R],
 *   rank[r] = #{c : x[r, c] > x[r, label]} + #{c < label : x[r, c] == x[r, label]}
 * exact integers; ties resolve towards the lower class index, so rank == 0 is np.argmax(x[r]) == label and `rank < k` is the top-k hit of
 * utils.accuracy (engine_for_finetuning.py:163,210) and of compute_video (:278-280): one launch serves Acc@1 and Acc@5.  Comparisons
 * with a NaN are false: a NaN logit outranks nothing (and a NaN at the label is outranked by nothing: rank 0).  labels are DEVICE data
 * and are not checked by the host; a label outside [0, C) reads nothing and gets rank C (a miss at every k). */
int tvts_class_ranks(const float* x, long ld, int R, int C, const int* labels, int* ranks, hipStream_t stream);
/* merge / compute_video (:231-285) on the device.  view_logits fp32 [N, V, C] (dense), seen uint8 [N, V] -> sum fp32 [N, C] (lds >= C)
 * and count int32 [N]: sum[n, c] = the fp32 sum of view_logits[n, v, c] over the views with seen[n, v] != 0, taken in the order
 * v = 0 .. V - 1 from +0.0f, every add rounded; no atomics: two runs give the same bits.  count[n] = the number of seen views.
 * compute_video takes the MEAN (:277); a mean and a sum rank identically (one positive divisor per video), so the division is left
 * out and the result feeds tvts_class_ranks as it is.  A video without a seen view gets a zero row and count 0: the caller leaves it
 * out of the average, as merge leaves out a video whose compute_video returns None (:265-268). */
int tvts_view_sum(const float* view_logits, const unsigned char* seen, int N, int V, int C, float* sum, long lds, int* count,
                  hipStream_t stream);
/* One batch of view logits into the buffers tvts_view_sum reads: row b of logits fp32 [B, C] (ld >= C) goes to view slot slot[b] =
 * video * V + view of view_logits fp32 [N * V, C], seen[slot] is set to 1 and video_labels[video] to labels[b].  merge keeps the FIRST
 * line of a (video, chunk, split) and skips the later ones (:251-252): a row whose slot is seen already, or named by an earlier row of
 * this batch, is dropped -- decided on the device from `seen`, without a host round trip.  slot / labels are DEVICE data; a slot
 * outside [0, N * V) drops its row. */
int tvts_view_store(const float* logits, long ld, int B, int C, const int* slot, const int* labels, int N, int V, float* view_logits,
                    unsigned char* seen, int* video_labels, hipStream_t stream);
/* torch.nn.utils.clip_grad_norm_ as v1/downstream/utils.py:366 calls it, without the host round trip: two-stage fixed-order sum of
 * squares over the 1024-element chunks of g whose chunk_group != 255 (partial: fp32 [nchunks] scratch), norm_coef[0] = norm =
 * |grad_scale| sqrt(sum), norm_coef[1] = coef = min(1, max_norm / (norm + 1e-6)), 1 when max_norm <= 0 (clipping off). */
int tvts_grad_sumsq(const float* g, const unsigned char* chunk_group, int nchunks, float* partial, float max_norm,
                    float grad_scale, float* norm_coef, hipStream_t stream);
/* The two torch rules of the v1 downstream steps, one launch over the flat store each.  Common to both: hyper_dev is the device
 * fp32 table lr[64] | wd[64]; chunk table as tvts_adamw_hf, groups 0..63, and a chunk of another group (255 = frozen) keeps every
 * bit of p, the state, the shadow and the average; the bf16 shadow (optional) is written in the same pass; g = stored gradient *
 * grad_scale * norm_coef[1] (norm_coef optional); the step count is `step`, or step_dev[0] when given (same device code, same bits).
 * -22 from either: p, g or a state stream the launch touches null or not 16-byte aligned; chunk_group or hyper_dev null;
 * nchunks <= 0; step <= 0 without step_dev; ema not 16-byte aligned, shadow / skipped not 8, step_dev / norm_coef not 4; under the
 * guard step_dev or norm_coef null; nesterov with momentum == 0.
 *
 * torch.optim.AdamW as optim_factory.py:129-130 builds it over the layer-decay groups of optim_factory.py:51-90: p *= 1 - lr wd;
 * m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g g; p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps), bias corrections in double. */
int tvts_adamw_torch(float* p, const float* g, float* m, float* v, void* shadow_bf16, const unsigned char* chunk_group, int nchunks,
                     const float* hyper_dev, int step, int* step_dev, double beta1, double beta2, double eps, float grad_scale,
                     const float* norm_coef, float* ema, float d32, float o32, long* skipped, hipStream_t stream);
/* torch.optim.SGD as optim_factory.py:121-126 builds it for v1/scripts/linear_ssv2.sh (--opt sgd --lr 0.1 --momentum 0.9
 * --weight_decay 1e-9: "sgd" / "nesterov" with nesterov=True, "momentum" without), single-tensor form of torch/optim/sgd.py with
 * dampening 0, bit for bit -- every add(x, alpha=a) there is one fused multiply-add:
 *   gg = g * gs; d = wd != 0 ? fmaf(wd, p, gg) : gg; momentum != 0: buf = first update ? d : fl(mu * buf) + d,
 *   d = nesterov ? fmaf(mu, buf, d) : buf; p = fmaf(-lr, d, p); shadow = bf16(p).
 * mu = fp32(momentum).  First update: the step count == 1; buf is then written, not read.  momentum == 0: buf is neither read nor
 * written and may be null. */
int tvts_sgd_torch(float* p, const float* g, float* buf, void* shadow_bf16, const unsigned char* chunk_group, int nchunks,
                   const float* hyper_dev, int step, int* step_dev, double momentum, int nesterov, float grad_scale,
                   const float* norm_coef, float* ema, float d32, float o32, long* skipped, hipStream_t stream);
/* The average (ema != null; null: none, d32 / o32 unused): timm.utils.ModelEma as run_class_finetuning.py:345-352 builds it and
 * engine_for_finetuning.py:84-85,97-98 updates it, per element ema = fl(fl(ema * d32) + fl(o32 * p)) -- three roundings, no FMA --
 * with d32 = fp32(decay) and o32 = fp32(1.0 - decay), the difference formed in double on the host.  The rule is applied to the
 * chunk's new p in the same pass; p, the state and the shadow get the bits of the launch without an average.  tvts_ema_update is the
 * rule as a pass of its own, with the same chunk gate (pointers 16-byte aligned, -22). */
int tvts_ema_update(float* ema, const float* p, const unsigned char* chunk_group, int nchunks, float d32, float o32,
                    hipStream_t stream);
/* The guard (skipped != null; null: unguarded): the overflow guard of the v1 fine-tuning step, GradScaler's "skip the update on
 * inf / NaN" decided on the device.  The update happens only when norm_coef[0] -- the global norm tvts_grad_sumsq left in device
 * memory, formed over the trainable chunks -- is finite.  Finite: step_dev[0] += 1 first, then the unguarded update with that step
 * count, bit for bit.  Not finite: every bit of p, the state, the shadow and the average is kept, step_dev[0] stays and the device
 * int64 skipped[0] += 1.  The step counter lives on the device only: step_dev and norm_coef are required, `step` is ignored. */
/* a[i] <-> b[i] in place and shadow_bf16[i] = bf16(new a[i]) for i < n; n % 4 == 0, a and b disjoint and 16-byte aligned (-22).
 * ModelEma.applied(): the masters and the average change places without a third buffer. */
int tvts_swap_f32_shadow(float* a, float* b, void* shadow_bf16, long n, hipStream_t stream);

/* ---- timing helper for bench.py: HIP events on the stream the kernels run on */
int tvts_event_create(void** ev);
int tvts_event_record(void* ev, hipStream_t stream);
int tvts_event_elapsed_ms(void* start, void* stop, float* ms);
int tvts_event_destroy(void* ev);
/* clock under load (SURVEY.md 8d "confirm the peak on the box: clocks x CUs x MFMA rate"): the rate of the constant counter
   (s_memrealtime) in kHz, the CU count and the sheet's maximum shader clock of the device; the shader cycles themselves are sampled
   INSIDE a GEMM launch (TVTS_GEMM_CLOCK_SAMPLE).  No reference site: the reference has no roofline accounting. */
/* p[0:nbytes] = 0 on the stream (a zero-fill kernel): optimizer.zero_grad() of the flat gradient buffer (v2/trainer/trainer.py:476) and
   the step's small accumulators */
int tvts_zero_bytes(void* p, long nbytes, hipStream_t stream);
int tvts_device_clock_info(int device, int* wall_clock_khz, int* cu_count, int* max_shader_khz);

#ifdef __cplusplus
}
#endif
#endif

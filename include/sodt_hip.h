/* C ABI of libsodt_hip.so -- the MI355X (gfx950) kernels beneath the reference's
 * Python nn.Module boundary (Model / ImageEncoderViT / C3 / Detect).
 *
 * The reference (Bissmella/Small-object-detection-transformers) has no FFI: every op
 * on its hot path is a torch.nn call.  Each entry point below therefore cites the
 * reference lines whose ATen op sequence it replaces (paths relative to the
 * reference root).  Conventions: raw device pointers + explicit sizes, caller-owned
 * memory (workspaces included), a hipStream_t argument, int return (SODT_OK;
 * SODT_EINVAL = the arguments were checked and refused, a shape or alignment the kernel does not support -- nothing launched
 * or written; SODT_ELAUNCH = the runtime failed a launch, an LDS opt-in, a memset or a sort -- earlier launches of the same
 * call may already be queued, none after it is), no allocation / synchronisation / exceptions inside; safe to capture in a
 * hipGraph.
 *
 * dtype: 0 = float32 (parity path, exact-f32 MFMA), 1 = bfloat16 (throughput path,
 * f32 accumulate).  Activations are token-major ("NHWC"): row = (b*H + y)*W + x,
 * channels contiguous.  Parameters handed to the kernels are the "prepared" copies
 * produced by sodt_prep_weights (cast to the run dtype, GEMM layouts [N][K]).
 */
#ifndef SODT_HIP_H
#define SODT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* sodt_stream_t;   /* == hipStream_t */

#define SODT_OK 0
#define SODT_EINVAL 1
#define SODT_ELAUNCH 2

#define SODT_F32 0
#define SODT_BF16 1
#define SODT_MAX_SEG 9

/* One K-segment of a GEMM's left operand: a (possibly spatially mapped) view of a
 * token-major tensor.  For output row m = (b, y, x) on the (Ho, Wo) grid the source
 * pixel is ((y*mul + dy) >> shr, (x*mul + dx) >> shr) on the (Hi, Wi) grid; rows
 * that fall outside read as zeros.  This one mechanism expresses the 2x2 conv of the
 * enhanced Swin MLP (backbone_vit.py:892-905), the 3x3 Bottleneck conv
 * (common.py:61), PatchMerging's 2x2 gather (backbone_vit.py:848-855),
 * nn.Upsample(x2, nearest) + Concat (models/model.yaml:66-72), channel concat of the
 * necks (backbone_vit.py:239,268) and every transposed (backward) form of them. */
typedef struct {
  const void* p;   /* base pointer, already offset to the first channel used */
  int ld;          /* row stride in elements */
  int klen;        /* channels taken from this segment (multiple of 16 bytes) */
  int dy, dx;      /* tap offset */
  int mul, shr;    /* stride multiply / upsample shift */
  int Hi, Wi;      /* source grid */
} sodt_seg;

typedef struct {
  sodt_seg s[SODT_MAX_SEG];
  int nseg;
  int spatial;     /* 0: source row == output row for every segment */
  int Ho, Wo;      /* output grid (rows = B*Ho*Wo) when spatial */
} sodt_aspec;

/* epilogue flags of sodt_gemm_nt */
#define SODT_EPI_BIAS 1          /* + bias[n] (f32) */
#define SODT_EPI_RESID 2         /* + R[m % rmod or m][n] */
#define SODT_EPI_GELU_DUAL 4     /* C = pre-activation, C2 = GELU(erf) of it */
#define SODT_EPI_DGELU 8         /* value *= gelu'(aux[m][n]) */
#define SODT_EPI_STATS 16        /* stats[r][0][n] += sum_m v, stats[r][1][n] += sum_m v*v (f64 atomics); the buffer holds
                                  * SODT_STATS_REPL replicas r of [2][N] (workgroups spread over them: same-address atomics
                                  * serialise in L2); sodt_bn_finalize sums the replicas */
#define SODT_STATS_REPL 16
#define SODT_EPI_AFFINE_SILU 32  /* v = silu(v*scale[n] + shift[n])  (fused / eval-mode Conv) */
#define SODT_EPI_DETECT 64       /* store f32 to (B, na, HW, no): Detect's view+permute */
#define SODT_EPI_OUT_F32 128
#define SODT_EPI_GELU 256        /* C = GELU(erf) of the value (after bias): fc1 when only the activation is kept */
#define SODT_EPI_DGELU_RC 512    /* two-phase K (bf16 pipelined kernel only): the first K/2 columns of A / W recompute the
                                  * pre-activation h = A1 W1^T (+ bias), the second K/2 give dh_act = A2 W2^T;
                                  * C = dh_act * gelu'(h).  Backward of Linear-GELU-Linear without saving h
                                  * (backbone_vit.py:886-904): A = [xn | dy], W = [fc1.weight | fc2.weight^T] */     /* C is float regardless of dtype */
#define SODT_EPI_RELU 2048       /* v = max(v, 0) after the bias: the ReLUs of the super-resolution branch (sr_decoder_noBN_noD.py:30-38,
                                  * edsr.py:44) */
#define SODT_EPI_DRELU 4096      /* v = aux[m][n] > 0 ? v : 0 - the gradient through a ReLU whose OUTPUT is aux (applied before RESID) */
/* (1024 was SODT_EPI_LNBWD, rounds 4-5: the LayerNorm backward as a GEMM epilogue - built, pinned, slower than the two launches it
 * replaced (profiles/r04_lnfold_ab.md) and removed in round 6; the bit is not reused) */

typedef struct {
  sodt_aspec a;                 /* A [M][K] as K-segments */
  const void* W; int ldw;       /* W [N][K], run dtype */
  void* C; int ldc;
  void* C2; int ldc2;
  const float* bias;
  const void* R; int ldr; int rmod;
  const void* aux; int ldaux;
  double* stats;                /* [2][N] */
  const float* scale; const float* shift;
  int M, N, K, flags;
  int oscatter, omul, ody, odx, OH, OW;   /* optional output-row scatter (PatchMerging backward) */
  int det_na, det_no, det_hw;
} sodt_gemm_args;

/* C = epilogue(A @ W^T): every nn.Linear / 1x1 / 2x2 / 3x3 Conv2d forward and every
 * input-gradient GEMM of the path (backbone_vit.py:968,990,886-904,857,213,268-270;
 * common.py:43,49; model.py:53). */
int sodt_gemm_nt(const sodt_gemm_args* g, int dtype, sodt_stream_t st);
/* test hook: which kernels sodt_gemm_nt / sodt_gemm_tn may choose (nt_route / tn_route in csrc/routes.h) */
#define SODT_VARIANT_AUTO 0      /* automatic */
#define SODT_VARIANT_TILED 1     /* NT: the K-loop 128 x 128 kernel; TN: the 128 x 128 kernel */
#define SODT_VARIANT_ASTAT 2     /* NT: A-stationary instead of B-stationary, no pipelined kernel; TN: without the pipelined kernel */
#define SODT_VARIANT_NO_TN3 3    /* NT as automatic; TN without the pipelined kernel */
int sodt_gemm_set_variant(int variant);

typedef struct {
  const void* dY; int ldy;      /* [M][N] run dtype; ldy >= N rounded up to 16 bytes (pad columns must be zero) */
  sodt_aspec x;                 /* X [M][K] as K-segments (same row mapping as the forward A) */
  float* dW; int lddw;          /* [N][K] f32, accumulated with atomics (zero it first) */
  float* dbias;                 /* [N] f32 or NULL: += column sums of dY */
  int M, N, K;
  int kperm_c, kperm_t;         /* if kperm_t > 1: column k = tap*C + ci is stored at ci*T + tap (torch conv layout) */
  int splits;                   /* M is cut into this many slices (grid.y) */
  float* partial;               /* optional f32 scratch of >= splits*N*K floats (16-byte aligned): the bf16 pipelined kernel then
                                 * writes one partial tile per slice with plain stores and a second kernel adds their sum to dW,
                                 * instead of splits*N*K contended atomics.  NULL / too small: atomics */
  long partial_floats;
} sodt_gemm_tn_args;

/* dW += dY^T @ X (+ dbias): every weight gradient of the path (autograd of the
 * reference ops listed above). */
int sodt_gemm_tn(const sodt_gemm_tn_args* g, int dtype, sodt_stream_t st);

/* Backward of a square 192 -> 192 nn.Linear in one pass over dY (csrc/linbwd.hip; autograd of backbone_vit.py:990 attn.proj and
 * :886-904 the conv-MLP's fc2), bf16 only:
 *   dX[M][192]   = epi(dY[M][192] @ W)      W given as wT [192][192] with wT[k][n] = W[n][k] - the [N][K] operand sodt_gemm_nt takes
 *   dW[192][192] (f32) += dY^T @ X[M][192]
 *   dbias[192]   (f32) += column sums of dY (NULL: skipped)
 * flags: 0, or SODT_EPI_DGELU: dX = (dY W) * gelu'(aux[m][k]) with the gelu' of sodt_gemm_nt's SODT_EPI_DGELU.
 * dY, X, aux, dX, wT: row-major bf16, 16-byte aligned, each leading dimension a multiple of 8 elements and >= 192; dW 16-byte aligned,
 * lddw a multiple of 4.  splits / partial / partial_floats: as in sodt_gemm_tn_args (M is cut into `splits` slices, one workgroup
 * each; with a scratch of >= splits*N*K floats the slices' partial tiles are summed in a fixed order - run-to-run deterministic -
 * otherwise dW gets f32 atomics; dbias goes through the scratch too when it has splits*N further floats).
 * N or K other than 192, float32, any other flag or alignment: SODT_EINVAL, nothing written (callers run sodt_gemm_tn + sodt_gemm_nt). */
typedef struct {
  const void* dY; int ldy;
  const void* X; int ldx;
  const void* wT; int ldw;
  const void* aux; int ldaux;
  void* dX; int lddx;
  float* dW; int lddw;
  float* dbias;
  int M, N, K, flags;
  int splits;
  float* partial;
  long partial_floats;
} sodt_linbwd_args;

int sodt_linear_bwd_sq(const sodt_linbwd_args* g, int dtype, sodt_stream_t st);

/* The same for the 192 -> 576 nn.Linear (csrc/linbwd.hip; autograd of backbone_vit.py:968 attn.qkv), bf16 only, N = 576, K = 192:
 *   dX[M][192]   = dY[M][576] @ W           wT [192][576], the [N][K] operand sodt_gemm_nt takes; bit-identical to its dX
 *   dW[576][192] (f32) += dY^T @ X[M][192]
 *   dbias[576]   (f32) += column sums of dY (NULL: skipped)
 * K is cut into three slabs of 64 columns and three workgroups share each of the `splits` M-slices (grid 3 * splits); each streams
 * the slice's dY rows, the second and third read being served by the L2 of their XCD.  flags must be 0.  Alignments, splits /
 * partial / partial_floats as above with N = 576 (splits * 576 * 192 floats of partial tiles, splits * 576 more for dbias);
 * ldy, ldw >= 576, ldx, lddx, lddw >= 192.  Anything else: SODT_EINVAL, nothing written (callers run sodt_gemm_tn + sodt_gemm_nt). */
int sodt_linear_bwd_wide(const sodt_linbwd_args* g, int dtype, sodt_stream_t st);

/* Backward of the linear MLP fc2(GELU(fc1(xn))) at C = 192, hidden 768, around one pass over xn and dY (csrc/mlpbwd.hip; autograd of
 * backbone_vit.py:884-890), bf16 only:
 *   h = xn[M][192] @ w1^T + b1 (recomputed, not stored)   w1 = fc1.weight [768][192], b1 = fc1.bias (f32)
 *   dh[M][768]    = (dY[M][192] @ fc2.weight) * gelu'(h)  w2T [768][192] with w2T[n][c] = fc2.weight[c][n], the [N][K] operand
 *                                                         sodt_gemm_nt takes; bit-identical to sodt_gemm_nt's SODT_EPI_BIAS |
 *                                                         SODT_EPI_DGELU_RC over [xn | dY] and [w1 | w2T]
 *   hact[M][768]  = GELU(h), sodt_mlp_fwd's logistic form (NULL: not written)
 *   dW1[768][192] += dh^T @ xn,      db1[768] += column sums of dh         (f32)
 *   dW2[192][768] += dY^T @ GELU(h), db2[192] += column sums of dY         (f32; GELU(h) rounded to bf16 as hact holds it)
 * The hidden dimension is cut into eight slabs of 96 columns and eight workgroups share each of the `splits` M-slices (grid
 * 8 * splits); each streams the slice's xn and dY rows, seven of the eight reads being served by the L2 of their XCD.
 * Every bf16 operand 16-byte aligned with a leading dimension that is a multiple of 8 elements and at least its width; the f32
 * operands 16-byte aligned, lddw1 >= 192 and lddw2 >= 768 multiples of 4.  partial / partial_floats: as in sodt_gemm_tn_args with
 * 2 * splits * 147,456 floats of partial tiles (summed in a fixed order: run-to-run deterministic) and splits * 960 more for the
 * two bias rows; a scratch too small for the tiles (or splits == 1): f32 atomics.
 * C other than 192, float32, a NULL operand other than hact, any other alignment: SODT_EINVAL, nothing written (callers run
 * sodt_gemm_tn + sodt_gemm_nt + sodt_gemm_tn).  The arguments are plain parameters, as sodt_mlp_fwd's. */
int sodt_mlp_bwd(const void* xn, int ldxn, const void* dY, int ldy, const void* w1, int ldw1, const float* b1,
                 const void* w2T, int ldw2, void* dh, int lddh, void* hact, int ldha, float* dW1, int lddw1, float* db1,
                 float* dW2, int lddw2, float* db2, long M, int C, int splits, float* partial, long partial_floats,
                 int dtype, sodt_stream_t st);

/* LayerNorm over the last dim, eps 1e-5 (backbone_vit.py:1090,1128,858).  y and stats
 * (mean, rstd per row, f32 [M][2]) are written; C % (16 bytes) == 0. */
int sodt_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* stats,
                       int M, int C, int dtype, sodt_stream_t st);
/* dx = [dres +] LN'(dy); dgamma/dbeta (f32) accumulated with atomics. */
int sodt_layernorm_bwd(const void* dy, const void* x, const float* stats, const float* gamma,
                       const void* dres, void* dx, float* dgamma, float* dbeta,
                       int M, int C, int dtype, sodt_stream_t st);

/* Window multi-head self-attention core on a natural-order QKV tensor
 * (backbone_vit.py:968-989 + :1094-1124): cyclic shift, window partition, q*scale@k^T,
 * relative-position bias, -100 shift mask, softmax, @v, un-partition, un-shift are all
 * index arithmetic inside the kernel.  qkv [B*H*W][3C], out [B*H*W][C], lse f32
 * [B*H*W][heads], bias_t f32 [heads][(2ws-1)^2] (transposed table).  Accepted geometry:
 * ws in {8, 16, 32, 64} dividing H and W, 0 <= shift < ws, head dim C/heads in {16, 32, 64},
 * and heads divisible by the waves per workgroup of the (dtype, head dim) instantiation
 * (forward: bf16 4/4/2, f32 4/2/2 for head dim 16/32/64; backward: bf16 4/2/1, f32 2/2/1).
 * Anything else returns SODT_EINVAL without writing. */
int sodt_window_attn_fwd(const void* qkv, const float* bias_t, void* out, float* lse,
                         int B, int H, int W, int C, int heads, int ws, int shift,
                         int dtype, sodt_stream_t st);
/* dqkv from dout (recomputes P); dbias_t accumulated with atomics; dq_acc is an f32
 * scratch of B*H*W*(C + heads) floats needed only when ws*ws > 64; its first B*H*W*C
 * floats must be zero on entry and are left zero on exit. */
int sodt_window_attn_bwd(const void* qkv, const float* bias_t, const void* out, const void* dout,
                         const float* lse, void* dqkv, float* dbias_t, float* dq_acc,
                         int B, int H, int W, int C, int heads, int ws, int shift,
                         int dtype, sodt_stream_t st);

/* The same attention core for a SHIFTED block whose H x W token grid is no multiple of its window (csrc/attention_sp.hip):
 * SwinTransformerBlock.forward backbone_vit.py:1094-1124 with the zero padding of window_partition / the crop of
 * window_unpartition :619-672 and the mask of :1058-1077, WindowAttention.forward :968-989.  The reference rolls the unpadded
 * grid by (-shift, -shift), zero-pads the rolled grid at the bottom / right AFTER norm1 (a pad token's q / k / v are qkv.bias),
 * attends per window of the padded grid with the mask's region ids taken from the unpadded rolled grid (pad positions: id 0),
 * crops and rolls back.  qkv [B*H*W][3C], out / dout [B*H*W][C], dqkv [B*H*W][3C] live on the UNPADDED grid in natural token
 * order; the padded grid is index arithmetic only.  qkv_bias f32 [3C]: what a pad key / value reads, narrowed to the run dtype
 * as a stored qkv row would be; a pad query is not computed into memory.  lse f32 [B*H*W][heads] (forward: may be NULL for
 * inference).  bias_t as above.  Accepted geometry: ws == 8, 0 < shift < 8, H > 8, W > 8, at least one of H, W no multiple
 * of 8, head dim 16 or 32, heads divisible by the waves per workgroup given above; everything else returns SODT_EINVAL and
 * launches nothing. */
int sodt_window_attn_sp_fwd(const void* qkv, const float* qkv_bias, const float* bias_t, void* out, float* lse,
                            int B, int H, int W, int C, int heads, int ws, int shift, int dtype, sodt_stream_t st);
/* dqkv from dout (recomputes P from lse; `out` is not read and may be NULL), written for every real token.  The k / v gradient
 * of the pad keys is ADDED to dqkv_bias (f32 [3C]; its q third is never touched); dbias_t accumulates as in
 * sodt_window_attn_bwd. */
int sodt_window_attn_sp_bwd(const void* qkv, const float* qkv_bias, const float* bias_t, const void* out, const void* dout,
                            const float* lse, void* dqkv, float* dqkv_bias, float* dbias_t,
                            int B, int H, int W, int C, int heads, int ws, int shift, int dtype, sodt_stream_t st);

/* ---- super-resolution auxiliary branch (deeplabedsr.py:35-73): data movement between its convolutions, token-major [B][H][W][C] ----
 * sodt_bilinear_up2_fwd/bwd: F.interpolate(x, size = (2H, 2W), mode = 'bilinear', align_corners = True) (sr_decoder_noBN_noD.py:37) and
 *   its adjoint (dx = sum over the output pixels a source pixel contributes to; written, not accumulated).  y / dy may be a
 *   column slice of a wider buffer (row stride ldy / lddy elements, pointer already at the slice); relu_out != NULL: x was the
 *   output of a ReLU ([B*H*W][C]) and dx is zeroed where it was not positive.
 * sodt_pixel_shuffle2: nn.PixelShuffle(2) (edsr.py:23): out[b][2y+i][2x+j][c] = in[b][y][x][4c + 2i + j], in [B][H][W][4C] ->
 *   out [B][2H][2W][C]; inverse != 0 runs the adjoint (= inverse permutation) out -> in.
 * sodt_add_rows: dst[m][dcol .. dcol + C) += src[m][scol .. scol + C) (gradient accumulation where a feature has two consumers); C, the
 *   leading dimensions and the column offsets are multiples of 16 bytes and both pointers 16-byte aligned - except ONE f32 row (M == 1)
 *   of fewer than 64 elements, which may have any width (the bias gradient of the 3-channel closing convolution).
 * sodt_nchw_f32_from_rows / sodt_rows_from_nchw_f32: y (B, C, H, W) f32 <-> token-major rows [B*H*W][ld] run dtype (C <= ld, the
 *   pad columns are written as zeros): the branch's output / its incoming gradient at the model boundary. */
int sodt_bilinear_up2_fwd(const void* x, void* y, int ldy, int B, int H, int W, int C, int dtype, sodt_stream_t st);
int sodt_bilinear_up2_bwd(const void* dy, int lddy, void* dx, const void* relu_out, int B, int H, int W, int C, int dtype,
                          sodt_stream_t st);
int sodt_pixel_shuffle2(const void* in, void* out, int B, int H, int W, int C, int inverse, int dtype, sodt_stream_t st);
int sodt_add_rows(void* dst, int ldd, int dcol, const void* src, int lds, int scol, long M, int C, int dtype, sodt_stream_t st);
int sodt_nchw_f32_from_rows(const void* rows, int ld, float* y, int B, int C, int H, int W, int dtype, sodt_stream_t st);
int sodt_rows_from_nchw_f32(const float* y, void* rows, int ld, int B, int C, int H, int W, int dtype, sodt_stream_t st);

/* ---- EDSR's closing convolution (edsr.py:81-84: conv(n_feats = 64, num_channels, 3) = nn.Conv2d(64, ch, 3, padding = 1), edsr.py:9-12),
 * forward and both gradients, on token-major rows (csrc/conv3.hip).  cout <= 8 output channels; bf16 only (SODT_EINVAL otherwise: the
 * float32 path runs the convolution as nine K-segments of sodt_gemm_nt / sodt_gemm_tn).  Each launch moves its tensors once.
 *   fwd:   y [B*H*W][8] = x [B*H*W][64] (*) w + bias; w [8][9*64] = [n][tap*64 + c] (tap = 3 ky + kx; rows >= cout zero), bias f32[8] or NULL.
 *          y_nchw != NULL: the result goes to (B, cout, H, W) float32 instead (the branch's output at the model boundary,
 *          deeplabedsr.py:73), unrounded; y is then unused and may be NULL.
 *   dgrad: dx [B*H*W][64] = dy (*)^T wT;  wT [64][9*8] = [c][tap*8 + n] (columns >= cout zero).  dy [B*H*W][8] bf16 (columns >= cout zero),
 *          or dy_nchw != NULL: (B, cout <= 4, H, W) float32, rounded to bf16 as it is read.
 *   wgrad: dw [cout][64][3][3] (the torch layout) += dy^T x(taps), db [cout] += column sums of dy (db may be NULL); dy / dy_nchw as above;
 *          scratch: sodt_conv3x3_c64n8_wgrad_scratch_bytes() bytes of f32 (per-workgroup partials, summed in a fixed order by a second launch). */
int sodt_conv3x3_c64n8_fwd(const void* x, const void* w, const float* bias, void* y, float* y_nchw, int B, int H, int W, int cout, int dtype,
                           sodt_stream_t st);
int sodt_conv3x3_c64n8_dgrad(const void* dy, const float* dy_nchw, const void* wT, void* dx, int B, int H, int W, int cout, int dtype,
                             sodt_stream_t st);
int sodt_conv3x3_c64n8_wgrad(const void* dy, const float* dy_nchw, const void* x, float* dw, float* db, float* scratch, int B, int H, int W,
                             int cout, int dtype, sodt_stream_t st);
long sodt_conv3x3_c64n8_wgrad_scratch_bytes(void);

/* ---- the 3x3 convolutions of EDSR at 64 input channels and 64 output channels per launch (edsr.py:34-53 ResBlock: conv -> ReLU -> conv,
 * + x; :64-70 head and body-closing convolutions; :14-24 Upsampler: conv(64 -> 256) + nn.PixelShuffle(2) as four launches), token-major
 * rows, bf16 only (csrc/conv3.hip): the input tile crosses the CU once, the weights live in registers.
 *   sodt_conv3x3_c64_fwd: y [B*H*W][64] = epilogue(x [B*H*W][64] (*) w); w [64][9*64] = [n][tap*64 + c].  flip != 0 mirrors the taps
 *     (tap' = 8 - tap): with w = the transposed weights [c][tap*64 + n] and x = dy this is the input gradient.  flags: any of
 *     SODT_EPI_BIAS (bias f32), SODT_EPI_RELU, and ONE of SODT_EPI_DRELU (aux [B*H*W][64]: keep where aux > 0) / SODT_EPI_RESID (resid
 *     [B*H*W][64]; may be y itself), applied in that order as in sodt_gemm_nt; anything else is SODT_EINVAL.
 *   sodt_conv3x3_c64_wgrad: dw [64][64][3][3] (torch layout) += dy^T x(taps), db [64] += column sums of dy (or NULL); scratch:
 *     sodt_conv3x3_c64_wgrad_scratch_bytes() bytes (per-workgroup partials, summed in a fixed order by a second launch).
 *   geo (NULL = identity): H x W is the grid the kernel walks.  Output channel n uses weight / bias (and dw / db) row
 *     w_row_stride * n + w_row_off; the input pixel (y, x) is read at (in_mul y + in_i, in_mul x + in_j) of an (in_mul H) x (in_mul W)
 *     tensor; the output pixel - and the epilogue operand, and dy of the weight gradient - at (out_mul y + out_i, out_mul x + out_j) of
 *     an (out_mul H) x (out_mul W) tensor; in_mul, out_mul in {1, 2}.  PixelShuffle(2) of a 64 -> 256 convolution = four launches with
 *     (w_row_stride, w_row_off, out_mul, out_i, out_j) = (4, 2 i + j, 2, i, j); its gradients read the fine gradient through the same map. */
typedef struct {
  int w_row_stride, w_row_off;
  int in_mul, in_i, in_j;
  int out_mul, out_i, out_j;
} sodt_conv3_geo;
int sodt_conv3x3_c64_fwd(const void* x, const void* w, const float* bias, const void* resid, const void* aux, void* y, int B, int H, int W,
                         int flags, int flip, const sodt_conv3_geo* geo, int dtype, sodt_stream_t st);
int sodt_conv3x3_c64_wgrad(const void* dy, const void* x, float* dw, float* db, float* scratch, int B, int H, int W, const sodt_conv3_geo* geo,
                           int dtype, sodt_stream_t st);
long sodt_conv3x3_c64_wgrad_scratch_bytes(void);

/* ---- fused W-MSA / SW-MSA half of a Swin block (csrc/wmsa_block.hip) -------------------------------------------
 * x_mid = x + Proj(WindowAttention(LN1(x))) and xn2 = LN2(x_mid) in ONE launch: SwinTransformerBlock.forward
 * backbone_vit.py:1084-1128 up to the MLP, with WindowAttention.forward :961-992, window_partition / unpartition
 * :619-672 and both torch.roll :1096,1118 as index arithmetic.  Built for the stage-1 geometry of model.yaml
 * (backbone_vit.py:117-133): C == 192, heads == 12 (head_dim 16), ws == 8, shift in [0, 8); H, W multiples of 8.
 * Any other shape returns SODT_EINVAL (callers fall back to sodt_layernorm_fwd + sodt_gemm_nt + sodt_window_attn_fwd).
 *
 * sodt_wmsa_pack: the block's raw f32 parameters -> the kernel's streaming order (per head: Wq/Wk/Wv rows and the
 *   Wproj column slice as MFMA fragments, the head's relative-position table x log2 e, q/k/v bias; then proj bias and
 *   the two LayerNorms), cast to the run dtype.  rpb_table is relative_position_bias_table as stored: ((2ws-1)^2, heads).
 *   wpk must hold sodt_wmsa_pack_bytes() bytes, 16-byte aligned.  Re-run whenever the parameters change.
 * sodt_wmsa_block_fwd: x, xm, xn2 [B*H*W][C] run dtype, natural token order.  Training passes the save-for-backward
 *   outputs (all or none): xn1 = LN1(x) [M][C]; st1 / st2 = (mean, rstd) of LN1 / LN2, f32 [M][2]; ao = attention
 *   output before the projection [M][C]; qkvw = q|k|v in window-major order [window][head][3][64][16] run dtype and
 *   lsew = log-sum-exp [window][head][64] f32, window = (b*(H/8) + wy)*(W/8) + wx in the shifted frame, token =
 *   window-local row-major - the operands of sodt_window_attn_bwd_wm.  Pass xn1 == NULL for inference.
 *   bf16: qkvw may be NULL (and the four-waves-per-window kernel never writes it): its backward, sodt_wmsa_block_bwd,
 *   recomputes q / k / v from xn1 and the pack; a non-NULL qkvw with bf16 returns SODT_EINVAL.  f32 (the parity path)
 *   requires qkvw. */
long sodt_wmsa_pack_bytes(int C, int heads, int ws, int dtype);
int sodt_wmsa_pack(const float* qkv_w, const float* qkv_b, const float* proj_w, const float* proj_b,
                   const float* rpb_table, const float* n1_w, const float* n1_b, const float* n2_w,
                   const float* n2_b, void* wpk, int C, int heads, int ws, int dtype, sodt_stream_t st);
int sodt_wmsa_block_fwd(const void* x, const void* wpk, void* xm, void* xn2, float* st1, float* st2,
                        void* xn1, void* qkvw, float* lsew, void* ao,
                        int B, int H, int W, int C, int heads, int ws, int shift, int dtype, sodt_stream_t st);
/* diagnostic hook: per-phase shader-cycle sums of the instrumented bf16 build (see csrc/wmsa_block.hip) */
int sodt_debug_wmsa_stamps(long long* out_host_256x8, int enable);
/* the same for the four-waves-per-window bf16 kernel (csrc/wmsa_hg.hip): 12 phases per workgroup */
int sodt_debug_wmsa_hg_stamps(long long* out_host_512x12, int enable);
/* sodt_window_attn_bwd on the window-major qkvw / lsew of sodt_wmsa_block_fwd (8x8 windows, head_dim 16);
 * dout and dqkv keep the natural layouts [M][C] / [M][3C]. */
int sodt_window_attn_bwd_wm(const void* qkvw, const float* bias_t, const void* dout, const float* lsew,
                            void* dqkv, float* dbias_t, int B, int H, int W, int C, int heads, int ws,
                            int shift, int dtype, sodt_stream_t st);
/* First stage of the fused block's backward, bf16 (backbone_vit.py:968 + the autograd of :971-989): d(attention output) dout
 * [M][C] -> dqkv [M][3C] and the relative-position-bias gradient dbias_t [heads][(2ws-1)^2] (accumulated), with q / k / v
 * RECOMPUTED per (window, head) from the block's saved LayerNorm-1 output xn1 [M][C] and its parameter pack wpk
 * (sodt_wmsa_pack) - the same MFMA product the forward ran - instead of read back from HBM; lsew as written by
 * sodt_wmsa_block_fwd.  C == 192, heads == 12, ws == 8, dtype == SODT_BF16 only; anything else returns SODT_EINVAL.  The
 * dgrad / wgrad GEMMs and the LayerNorm backward of the block stay separate launches (sodt_gemm_nt / _tn, sodt_layernorm_bwd). */
int sodt_wmsa_block_bwd(const void* xn1, const void* wpk, const float* bias_t, const void* dout, const float* lsew,
                        void* dqkv, float* dbias_t, int B, int H, int W, int C, int heads, int ws, int shift,
                        int dtype, sodt_stream_t st);

/* ---- fused linear MLP of a Swin block (csrc/mlp.hip) -----------------------------------------------------------
 * out = resid + fc2(GELU(fc1(xn))): Mlp.forward's linear branch backbone_vit.py:884-890 (fc1, exact-erf GELU, fc2; the
 * dropouts are identities at p = 0) together with the block's residual add `x + drop_path(mlp(norm2(x)))` (:1128), ONE launch.
 * xn, resid, out [M][C] run dtype (resid nullable: then out = fc2(GELU(fc1(xn)))); w1 = fc1.weight [4C][C], w2 = fc2.weight
 * [C][4C] in the run dtype (the prepared [N][K] copies sodt_gemm_nt takes), b1 [4C] / b2 [C] f32.
 * hact (nullable): GELU(fc1(xn) + b1) [M][4C] run dtype is also written - the operand of fc2's weight gradient; without it the
 * 4C-wide hidden activation never leaves the CU (inference form).
 * bf16, C == 192: the fused kernel (token tile in LDS, W1 / W2 streamed in 32-column slabs by LDS-DMA, GELU(h) chained from the
 * first product's accumulators into the second product's operand).  f32 (the parity path) and every other width run the
 * two-launch chain sodt_gemm_nt(GELU) -> sodt_gemm_nt(bias + residual) through hact, which is then required. */
int sodt_mlp_fwd(const void* xn, const void* w1, const float* b1, const void* w2, const float* b2, const void* resid,
                 void* out, void* hact, long M, int C, int dtype, sodt_stream_t st);

/* ---- 2x2-conv MLP of the shifted Swin blocks with fc1 folded into the convolution (csrc/convmlp.hip), bf16 -------------------
 * Mlp.forward's convolutional branch, backbone_vit.py:892-905: fc1 (C -> C), F.pad right / bottom, conv1 (2x2), GELU, fc2.  conv1 o fc1 is
 * one linear map per tap, so the 2x2 convolution runs directly on the LayerNorm output with composed weights and bias; the tokens of
 * the last column / row (where the padded fc1 output is zero including its bias) get a correction.  Exact algebra, bf16 rounding
 * differs (fc1's output is never rounded).  f32 masters in their torch layouts: fc1_w [C][C], conv_w [C][C][2][2] (tap = kh * 2 + kw).
 * sodt_convmlp_compose: weff bf16 [C][4C] (column tap * C + ci: the W operand of sodt_gemm_nt over the four tap segments), weffT bf16
 *   [C][4C] (row ci, column tap * C + co: the W operand of the input-gradient GEMM over the negated taps), beff f32 [C] = conv bias +
 *   sum_taps Wc_tap b1, vtap f32 [4][C] = Wc_tap b1.  Run once per forward (the masters change every step).
 * sodt_convmlp_border_fix: cp (pre-activation) and ca (GELU of it) [B*H*W][C] as written by the GEMM with beff: on the tokens with
 *   x == W - 1 / y == H - 1 the taps outside the image lose their vtap again and ca is recomputed.
 * sodt_convmlp_border_sums: bs f32 [3][C] (zeroed by the caller) += sums of dc [B*H*W][C] over the last-column tokens, the last-row
 *   tokens and the corner tokens.
 * sodt_convmlp_decompose: parameter gradients by the chain rule from dweff f32 [C][4C] (= dc^T x(taps), sodt_gemm_tn without kperm),
 *   colsum f32 [C] (its dbias) and bs: g_conv_w [C][C][2][2], g_conv_b, g_fc1_w, g_fc1_b are ADDED to.  C <= 384.
 * Reproducibility: sodt_convmlp_border_sums and the fc1.weight part of sodt_convmlp_decompose sum their per-workgroup partials with
 *   f32 atomicAdd (four k-quarters per tile / one partial per 8-token chunk), so g_fc1_w, g_fc1_b and g_conv_w of a folded MLP agree
 *   run to run only to f32 summation order (~1e-7 relative) - unlike the weight gradients of sodt_gemm_tn and the direct 3x3 kernels,
 *   which reduce their partial tiles in a fixed order and are bitwise reproducible. */
int sodt_convmlp_compose(const float* fc1_w, const float* fc1_b, const float* conv_w, const float* conv_b, void* weff, void* weffT,
                         float* beff, float* vtap, int C, int dtype, sodt_stream_t st);
int sodt_convmlp_border_fix(void* cp, void* ca, const float* vtap, int B, int H, int W, int C, int dtype, sodt_stream_t st);
int sodt_convmlp_border_sums(const void* dc, float* bs, int B, int H, int W, int C, int dtype, sodt_stream_t st);
int sodt_convmlp_decompose(const float* dweff, const float* colsum, const float* bs, const float* fc1_w, const float* fc1_b,
                           const float* conv_w, float* g_conv_w, float* g_conv_b, float* g_fc1_w, float* g_fc1_b, int C, sodt_stream_t st);

/* Front end (backbone_vit.py:195-210): channel split, 4x Conv2d(1->48,k4,s4) (R with
 * padding 1), pairwise cross-channel attention (R<-G, G<-B, B<-IR, IR<-G; 12 heads x 4,
 * scale 1/2, window ca_ws, no projections) + residual + LayerNorm(48), concatenated to
 * [B*th*tw][192], th x tw = H/4 x W/4 tokens, output row (b * th + y) * tw + x.  rgb (B,3,H,W) f32 / ir plane pointer with
 * its batch stride, f32 in [0,1].  params f32: w[4][48][16], b[4][48], gamma[4][48], beta[4][48].  ca_ws == 1
 * is the shipped configuration (backbone_vit.py:438).  H % 4 or W % 4 non-zero is refused (SODT_EINVAL, nothing launched):
 * the patches are 4 x 4 and are read as 16-byte rows.
 * The backward accumulates into dw/db/dgamma/dbeta.  With a workspace of sodt_frontend_bwd_workspace_bytes() (f32, need
 * not be zeroed) the per-workgroup partial sums are reduced by a second small kernel; ws == NULL falls back to direct
 * atomics (same result up to summation order, ~0.15 ms slower at 8 x 1024^2). */
int sodt_frontend_fwd(const float* rgb, const float* ir, long ir_bstride, const float* w, const float* b,
                      const float* gamma, const float* beta, void* out, int B, int H, int W, int ca_ws,
                      int dtype, sodt_stream_t st);
long sodt_frontend_bwd_workspace_bytes(int B, int H, int W);
int sodt_frontend_bwd(const float* rgb, const float* ir, long ir_bstride, const float* w, const float* b,
                      const float* gamma, const float* beta, const void* dout,
                      float* dw, float* db, float* dgamma, float* dbeta, int B, int H, int W, int ca_ws,
                      float* ws, long ws_bytes, int dtype, sodt_stream_t st);

/* General cross-channel attention (window ca_ws in 1..8, optional cyclic shift; backbone_vit.py:469-561, :589-616) as
 * separate stages: e = 4x Conv2d(1->48,k4,s4) embeddings, f32 [B*th*tw][192] (caller's workspace); then per pair
 * softmax((q k^T + mask)/2) v + residual + LayerNorm(48).  The roll and the 0 / -100 mask run per axis on the th x tw grid;
 * refused unless H % 4 == W % 4 == 0 and both th and tw are multiples of ws.  The backward accumulates d e with atomics
 * (zero it first); dw/db/dgamma/dbeta accumulate.  ca_ws == 1 callers should use the fused sodt_frontend_* instead. */
int sodt_patch_embed4_fwd(const float* rgb, const float* ir, long ir_bstride, const float* w, const float* b,
                          float* e, int B, int H, int W, sodt_stream_t st);
int sodt_patch_embed4_bwd(const float* rgb, const float* ir, long ir_bstride, const float* de, float* dw, float* db,
                          int B, int H, int W, sodt_stream_t st);
int sodt_cross_attn_ln_fwd(const float* e, const float* gamma, const float* beta, void* out, int B, int H, int W, int ws,
                           int shift, int dtype, sodt_stream_t st);
int sodt_cross_attn_ln_bwd(const float* e, const float* gamma, const void* dout, float* de, float* dgamma,
                           float* dbeta, int B, int H, int W, int ws, int shift, int dtype, sodt_stream_t st);

/* BatchNorm2d (eps 1e-3, momentum 0.03) + SiLU of the head's Conv (common.py:38-50,
 * torch_utils.py:150-152), token-major.  stats f64 [SODT_STATS_REPL][2][C] from SODT_EPI_STATS.
 * finalize: mean/rstd (f32 [2][C]) + running-stat update (unbiased var); stats == NULL
 * takes mean/rstd from the running statistics (eval).
 * sodt_col_stats: the same statistics from a STORED convolution output z [M][ldz] (stats[r][0][c] += sum_m z, stats[r][1][c] += sum_m z^2,
 * f64, one replica r per workgroup) - for the convolutions that run on the direct 3x3 kernels (csrc/conv3.hip), which have no
 * statistics epilogue. */
int sodt_col_stats(const void* z, int ldz, double* stats, long M, int C, int dtype, sodt_stream_t st);
int sodt_bn_finalize(const double* stats, float* mean_rstd, float* running_mean, float* running_var,
                     long count, int C, float eps, float momentum, sodt_stream_t st);
/* scale = gamma*rstd, shift = beta - mean*scale: the fused / eval-mode form (torch_utils.py:182-203) */
int sodt_bn_affine(const float* mean_rstd, const float* gamma, const float* beta, float* scale, float* shift,
                   int C, sodt_stream_t st);
/* The three BatchNorm+SiLU launches take rows of at most 256 16-byte chunks (C <= 2048 in bf16, 1024 in f32): a thread keeps one
   chunk of the row for the whole launch.  Wider rows return SODT_EINVAL. */
int sodt_bn_silu_fwd(const void* z, const float* mean_rstd, const float* gamma, const float* beta,
                     void* y, int ldy, long M, int C, int dtype, sodt_stream_t st);
/* pass 1: red[0][c] += sum g, red[1][c] += sum g*xhat with g = dy * silu'(a);  pass 2: dz, rows lddz elements apart (dense: C;
   a column slice of a wider buffer: the pointer carries the column offset, as dy's does) */
int sodt_bn_silu_bwd_reduce(const void* dy, int lddy, const void* z, const float* mean_rstd,
                            const float* gamma, const float* beta, double* red, long M, int C,
                            int dtype, sodt_stream_t st);
int sodt_bn_silu_bwd_apply(const void* dy, int lddy, const void* z, const float* mean_rstd,
                           const float* gamma, const float* beta, const double* red, void* dz,
                           float* dgamma, float* dbeta, long M, int C, int lddz, int dtype, sodt_stream_t st);
/* pass 2 where the BatchNorm statistics are shared by data-parallel ranks (torch.nn.SyncBatchNorm, Train.py:206-209): the two means
   of dz are red_global / count_total - the sums of every rank's rows (red_local after its all-reduce) over the rows of all
   ranks - while dgamma / dbeta += (float)red_local, this rank's own sums: the gradient all-reduce combines those like every other
   gradient.  red_global == red_local and count_total == M give sodt_bn_silu_bwd_apply bit for bit.  count_total >= M. */
int sodt_bn_silu_bwd_apply_sync(const void* dy, int lddy, const void* z, const float* mean_rstd,
                                const float* gamma, const float* beta, const double* red_local,
                                const double* red_global, long count_total, void* dz, float* dgamma, float* dbeta,
                                long M, int C, int lddz, int dtype, sodt_stream_t st);

/* dst[(b,y,x)][coff : coff+C] = src[(b, y>>shr, x>>shr)][0:C]  (nn.Upsample nearest + Concat slot) */
int sodt_copy_rows(const void* src, int lds_, void* dst, int ldd, int B, int Ho, int Wo, int shr, int C,
                   int dtype, sodt_stream_t st);
/* dsrc[(b,y,x)][c] (+)= sum_{a,b<2^shr} d[(b, (y<<shr)+a, (x<<shr)+b)][c]  (their backward) */
int sodt_gather_sum_rows(const void* d, int ldd, void* dsrc, int lds_, int B, int Hs, int Ws, int shr, int C,
                         int accumulate, int dtype, sodt_stream_t st);

/* nn.MaxPool2d(5, stride 1, padding 2), token-major, the unit of SPP (common.py:129-140: its 5 / 9 / 13 pools are this pool
 * applied 1 / 2 / 3 times).  argmax (nullable in inference): one byte per (token, channel), window slot ky*5+kx of the
 * first maximum in scan order of THAT 5x5 window (PyTorch's rule for a 5x5 pool; for the cascaded 9 / 13 pools ties inside
 * the composed window may resolve to a different, equally valid, tied element than torch's single 9x9 / 13x13 scan).
 * bwd: dx (+)= gather of dy through argmax. */
int sodt_maxpool5_fwd(const void* x, int ldx, void* y, int ldy, unsigned char* argmax, int B, int H, int W, int C,
                      int dtype, sodt_stream_t st);
int sodt_maxpool5_bwd(const void* dy, int lddy, const unsigned char* argmax, void* dx, int lddx, int accumulate,
                      int B, int H, int W, int C, int dtype, sodt_stream_t st);

/* Detect: dpred f32 (B, na, HW, no) -> dz run dtype [B*HW][ldz] (cols >= na*no zeroed)  (model.py:55 backward) */
int sodt_detect_unpermute(const float* dpred, void* dz, int ldz, int B, int HW, int na, int no,
                          int dtype, sodt_stream_t st);
/* Detect eval decode (model.py:61-64): raw f32 (B,na,ny,nx,no) -> z f32 (B, na*ny*nx, no) */
int sodt_detect_decode(const float* raw, const float* anchor_grid, float* z, int B, int na, int ny, int nx,
                       int no, float stride, sodt_stream_t st);

/* Test-time augmentation (csrc/tta.hip; basics/models/model.py:155-184, the `--augment` of basics/test.py).
 *
 * sodt_tta_scale makes every augmented input of one call in ONE launch.  Per pass it replaces, for the RGB and the IR batch,
 * `x.flip(fi)` (model.py:161-162), `F.interpolate(img, size=(int(h * ratio), int(w * ratio)), mode='bilinear',
 * align_corners=False)` and `F.pad(img, [0, Wp - w, 0, Hp - h], value=0.447)` (torch_utils.py:254-259).  rgb / ir: f32
 * (B, c, H, W) contiguous (device); c_ir may be 0 (ir and every out_ir then unused).  passes: a HOST table of npass <=
 * SODT_TTA_MAX_PASSES entries that travels to the kernel by value: out_rgb / out_ir f32 (B, c, Hp, Wp); (h, w) the content size
 * the input is resized to, (Hp, Wp) >= (h, w) the padded size; flip 0, 2 (up-down) or 3 (left-right), applied to the source
 * coordinate, i.e. before the resize.  Source index and blend weight come from the exact integer quotient and remainder of
 * max((2 o + 1) * in - out, 0) / (2 * out); every output element is written, the pixels outside (h, w) as 0.447f; (h, w) ==
 * (H, W) is the flipped copy bit for bit.
 * SODT_EINVAL, nothing launched: a null pointer, a non-positive size, batch or c_rgb (c_ir < 0), h > Hp or w > Wp, a flip
 * outside {0, 2, 3}, npass outside 1 .. SODT_TTA_MAX_PASSES, or one of H * W, 2 * h * H, 2 * w * W reaching 2^31. */
#define SODT_TTA_MAX_PASSES 4
typedef struct {
  float* out_rgb; float* out_ir;
  int h, w;                  /* content size */
  int Hp, Wp;                /* padded size */
  int flip;                  /* 0, 2 = up-down, 3 = left-right */
} sodt_tta_pass;
int sodt_tta_scale(const float* rgb, const float* ir, int B, int c_rgb, int c_ir, int H, int W, const sodt_tta_pass* passes,
                   int npass, sodt_stream_t st);

/* sodt_detect_decode for one pass of the augmented forward, written into its slice of the concatenated output with the
 * de-scale and the de-flip of model.py:178-182 applied: rows row_off .. row_off + na*ny*nx of z f32 (B, rows_total, no) get the
 * decoded values (the same arithmetic as sodt_detect_decode, shared source), columns 0..3 divided by si (IEEE f32 division,
 * what `yi[..., :4] /= si` is on ATen's CPU path), then x = (float)img_w - x for flip 3, y = (float)img_h - y for flip 2
 * (img_h, img_w: the ORIGINAL input's size).  Rows outside the slice are not touched.
 * SODT_EINVAL, nothing launched: what sodt_detect_decode refuses, row_off < 0, a slice that ends past rows_total, si not a
 * positive finite number, a flip outside {0, 2, 3}, a non-positive img_h or img_w, na * ny * nx * no reaching 2^31 (the index
 * inside one image is 32-bit), B > 65535. */
int sodt_detect_decode_tta(const float* raw, const float* anchor_grid, float* z, int B, int na, int ny, int nx, int no,
                           float stride, long row_off, long rows_total, float si, int flip, int img_h, int img_w,
                           sodt_stream_t st);

/* The Detect level in one pass each way (csrc/detect.hip; model.py:44-58 and its autograd), bf16 only.  M = B * HW rows, N = na * no:
 *   sodt_detect_fwd   pred[b][a][p][o] (f32) = X[b*HW + p][0:K] . W[a*no + o][0:K] + bias[a*no + o]  - what sodt_gemm_nt computes
 *                     with SODT_EPI_DETECT | SODT_EPI_BIAS (same products, same K order), written as whole runs of pred
 *   sodt_detect_bwd   dZ[m][n] = bf16(pred[b][a][p][o]) (pred holds d(pred) here; the rounding of sodt_detect_unpermute), then
 *                     dX[M][K] (bf16) = dZ @ W;  dW[N][K] (f32) += dZ^T @ X;  dbias[N] (f32) += column sums of dZ (NULL: skipped)
 *                     flags: SODT_DETECT_NO_WGRAD leaves dW / dbias alone, SODT_DETECT_NO_DX leaves dX alone (not both).
 *                     With dW the caller gives a scratch of >= splits * (48 K + 48) floats: every slice leaves its partial there
 *                     and a second kernel adds the live slices to dW / dbias in a fixed order (run-to-run deterministic; equal
 *                     to sodt_gemm_tn's result up to f32 summation order).
 * X, W, dX: row-major bf16, 16-byte aligned, leading dimensions multiples of 8 and >= K; pred, bias, dW, dbias, partial 16-byte
 * aligned, lddw a multiple of 4 and >= K.  splits: M is cut into this many slices of whole 32-row stages, one workgroup each.
 * K not a multiple of 32 or beyond 256, na * no > 48, float32, an alignment off, a scratch too small: SODT_EINVAL, nothing
 * launched or written (callers run sodt_gemm_nt / sodt_detect_unpermute + sodt_gemm_tn + sodt_gemm_nt). */
#define SODT_DETECT_NO_WGRAD 1
#define SODT_DETECT_NO_DX 2
typedef struct {
  const void* X; int ldx;
  const void* W; int ldw;
  const float* bias;
  float* pred;
  void* dX; int lddx;
  float* dW; int lddw;
  float* dbias;
  int B, HW, na, no, K, flags;
  int splits;
  float* partial;
  long partial_floats;
} sodt_detect_args;
int sodt_detect_fwd(const sodt_detect_args* g, int dtype, sodt_stream_t st);
int sodt_detect_bwd(const sodt_detect_args* g, int dtype, sodt_stream_t st);

/* ---- non_max_suppression (general.py:425-512), one image per call, eval only ---------------------------
 * z: decoded rows (N, 5+nc) f32 [cx cy w h obj cls...] of one image (Detect eval output, model.py:64).
 * sodt_nms_candidates: general.py:433,446-476 - rows with obj > conf; multi_label (forced off when nc == 1):
 *   one candidate per class with obj*cls > conf, else the best class; class_allow (nc bytes, device, nullable)
 *   is the `classes` filter (general.py:479-480).  Writes *count (device int, may exceed cap - then the call must
 *   be repeated with a larger cap) and one 64-bit key per candidate, (~score_bits << 32) | (row*nc + class).
 * sodt_nms_select: sorts the keys (descending score, ties in the reference's candidate order), keeps the top
 *   30000 (general.py:489-490), runs class-offset NMS at iou_thres (torchvision.ops.nms semantics,
 *   general.py:493-496), cuts at 300 (general.py:497-498), merge-NMS + redundancy filter when
 *   1 < n_total < 3000 (general.py:499-506).  out: (<=300, 6) f32 [x1 y1 x2 y2 conf cls]; out_index: the
 *   candidate id row*nc + class of each output row; *out_count: rows written.  ws: scratch of at least
 *   sodt_nms_workspace_bytes(n_total).  Nothing synchronises; the caller reads *count / *out_count. */
int sodt_nms_candidates(const float* z, int N, int nc, float conf_thres, int multi_label,
                        const unsigned char* class_allow, unsigned long long* keys, int cap, int* count,
                        sodt_stream_t st);
int sodt_nms_workspace_bytes(long n_total, size_t* bytes);
int sodt_nms_select(const float* z, int nc, const unsigned long long* keys, long n_total, float iou_thres,
                    int agnostic, void* ws, size_t ws_bytes, float* out, int* out_index, int* out_count,
                    sodt_stream_t st);

/* ---- non_max_suppression (general.py:425-512), a whole batch per call, no host read, eval only ---------------
 * The batched sibling of the three entries above: the same candidates, the same 64-bit key, the same result per image.
 * z: decoded rows (B, N, 5+nc) f32.  labels / nlab / lab_cap (all null / 0, or all set): the autolabelling rows of
 *   general.py:451-458, labels (B, lab_cap, 5) f32 [cls x y w h] of which image b uses the first nlab[b] (device int32,
 *   clamped to lab_cap); they are candidates' rows N + k with obj = 1 and a one-hot class, read in place - no
 *   concatenated prediction exists.  A label whose class is not in [0, nc) has no class score.
 * conf_thres / iou_thres / multi_label (forced off when nc == 1) / class_allow (nc bytes, device, nullable) / agnostic:
 *   as sodt_nms_candidates and sodt_nms_select (general.py:425-512).
 * Per image: candidates into a key segment of rows * (multi_label ? nc : 1) slots (rows = N + lab_cap), ONE segmented
 *   radix sort (descending score, ties in the reference's candidate order), the first 30000 survive (general.py:489-490),
 *   greedy class-offset NMS that stops at 300 kept (torchvision.ops.nms then i[:max_det], general.py:493-498), merge-NMS
 *   and the redundancy filter where 1 < candidates < 3000 (general.py:499-506).
 * out_rows: (B*300, 6) f32 [x1 y1 x2 y2 conf cls], image b's rows at [out_off[b], out_off[b+1]); out_index: (B*300) int32,
 *   the candidate id row*nc + class of each row; out_off: (B+1) int32, written on the device.  Rows and ids from
 *   out_off[B] to B*300 are zeros.  This is the packed (det, det_off) form of sodt_eval_match / sodt_confusion_update with
 *   n_det = B*300 as the upper bound.
 * ws: 16-byte aligned scratch of at least sodt_nms_batch_workspace_bytes(B, N + lab_cap, nc, multi_label): a function
 *   of these host-known arguments alone.  B <= 4096, rows * nc and B * slots below 2^31.
 * Neither entry allocates, synchronises or reads device memory on the host; arguments are checked before the first
 *   launch (SODT_EINVAL, nothing written); the launches are the same for every B and every count. */
int sodt_nms_batch_workspace_bytes(int B, long rows, int nc, int multi_label, size_t* bytes);
int sodt_nms_batch(const float* z, int B, int N, int nc, const float* labels, const int* nlab, int lab_cap,
                   float conf_thres, float iou_thres, int multi_label, const unsigned char* class_allow, int agnostic,
                   void* ws, size_t ws_bytes, float* out_rows, int* out_index, int* out_off, sodt_stream_t st);

/* ---- weighted boxes fusion (general.py:515-563, ensemble_boxes/ensemble_boxes_wbf.py), a batch per call, eval only ----
 * sodt_wbf_candidates: general.py:523-544 for all B images in one launch.  z: (B, N, 5+nc) f32.  Keeps rows with
 *   obj > conf_thres whose best class (first maximum of the f32 product obj * cls) has obj * cls > conf_thres, divides
 *   cx cy w h by image_size (a true f32 division) and converts to corners in f32 (xywh2xyxy).  Per image b it writes, in
 *   no particular order, boxes (B, N, 4) f32 [x1 y1 x2 y2] (16-byte aligned), scores (B, N) f32, labels (B, N) int32,
 *   src (B, N) int32 = the row the candidate came from, and counts[b] (device int32) = rows of image b written.
 * sodt_wbf_fuse: weighted_boxes_fusion (ensemble_boxes_wbf.py:150-225) for B images at once.  Image b owns rows
 *   [b*cap, b*cap + counts[b]) of boxes (f32 corners, 16-byte aligned) / scores / labels / model / src.  model: int32
 *   model index of each row, NULL = model 0; rows whose model is outside [0, n_models) are dropped.  src: int32 tie-break
 *   index, NULL = the row's position.  weights: a HOST array of n_models <= 32 doubles.  conf_type: 0 avg, 1 max,
 *   2 box_and_model_avg, 3 absent_model_aware_avg.  Rows with score < skip_box_thr (an f32 comparison) are dropped
 *   (:31-102); the weighted score is the f64 product score * weights[model].  Within an image the rows are walked by
 *   label, then descending weighted score, then ascending src (the reference's argsort()[::-1] leaves ties unordered).
 *   Clustering (:183-195, find_matching_box :135-147, bb_intersection_over_union :11-28): a row joins the cluster whose
 *   box has the greatest IoU strictly above iou_thr (f64), the earliest cluster among equal IoUs, else it starts one.
 *   Cluster arithmetic is get_weighted_box's (:105-132): f32 coordinate sums updated as (float)((double)acc + s * x), the
 *   score sum in f64, the fused coordinate (float)((double)acc / sum), the IoU of the f32 boxes in f64.  Confidence as
 *   :196-218 for all four conf_type values and both allows_overflow values.  Output per image (:219-225): clusters by
 *   descending score (ties: label, then creation order) in out_boxes (B, cap, 4) f32 (16-byte aligned), out_scores
 *   (B, cap) f32, out_labels (B, cap) int32; out_counts[b] (device int32) = clusters of image b.  member (nullable,
 *   (B, cap) int32): for each input row the output row of its cluster within its image, -1 for a dropped row.
 *   scan_lanes: lanes of the workgroup that walks one (image, label) segment, 64 or 256; 0 = the default.
 *   ws: 256-byte aligned scratch of at least sodt_wbf_fuse_workspace_bytes(B, cap) (one cluster per row at worst).
 *   B <= 65535, B * cap <= 2^30.  No entry allocates or synchronises.  Every argument is checked before the first launch
 *   (SODT_EINVAL); a failing runtime call (a memset, a rocPRIM sort, a launch) returns SODT_ELAUNCH part-way, and only then
 *   may earlier launches of the same call already be queued. */
int sodt_wbf_candidates(const float* z, int B, int N, int nc, float conf_thres, float image_size, float* boxes,
                        float* scores, int* labels, int* src, int* counts, sodt_stream_t st);
int sodt_wbf_fuse_workspace_bytes(int B, long cap, size_t* bytes);
int sodt_wbf_fuse(const float* boxes, const float* scores, const int* labels, const int* model, const int* src,
                  const int* counts, int B, long cap, const double* weights, int n_models, double iou_thr,
                  float skip_box_thr, int conf_type, int allows_overflow, int scan_lanes, void* ws, size_t ws_bytes,
                  float* out_boxes, float* out_scores, int* out_labels, int* out_counts, int* member, sodt_stream_t st);

/* ---- validation statistics (basics/test.py:155-264, basics/utils/metrics.py:18-106), eval only ----------------
 * sodt_eval_match: the per-image true-positive matching of test.py:155-240 for a whole batch at once.
 *   det: the NMS rows of all images packed, (n_det, 6) f32 [x1 y1 x2 y2 conf cls] in letterboxed-input pixels;
 *   det_off: (B+1) device int32 image offsets into det.  targets: (nt, 6) f32 [img cls x y w h] in input pixels
 *   (test.py:149), in any order - grouped by image on the device, each image's rows kept in their order.
 *   geom: (B, 5) f32 [h0 w0 gain padw padh] per image (scale_coords' img0_shape and ratio_pad, general.py:323-336).
 *   iouv: the 10 IoU thresholds, a HOST array (torch.linspace(0.5, 0.95, 10), test.py:100).
 *   correct: (n_det, 10) uint8, test.py:206-237 bit for bit (scale_coords of predictions and xywh2xyxy'd labels,
 *   box_iou, max(1) with the lowest target index on ties, the greedy per-class walk in NMS row order, iou > iouv).
 *   tcls_out: (nt) f32, the target classes in image order (test.py:159's tcls concatenated); rows whose image index is
 *   not an integer in [0, B) match nothing and are written as -1.  Any number of labels per image.
 *   ws: scratch of at least sodt_eval_match_workspace_bytes(B, n_det, nt).
 * sodt_ap_per_class: ap_per_class + compute_ap (metrics.py:18-106) in f64.  tp (n, 10) uint8, conf / pred_cls (n) f32,
 *   target_cls (nt) f32; classes are integral values in [0, nc), nc <= 4096.  Negative target classes are padding and
 *   ignored; other target classes outside [0, nc) are counted in info[1] (the result is then not the reference's);
 *   predictions of a class no target has are ignored, as in the reference.  Outputs, first info[0] = nc_u rows valid:
 *   p, r, f1 (nc) f64 at the first argmax of f1.mean(0); ap (nc, 10) f64; classes (nc) int32 = np.unique(target_cls);
 *   nt_count (nc) int32 = np.bincount(target_cls, minlength=nc) (test.py:261).  info: int32[4] =
 *   [nc_u, bad target classes, rows of tp with any true entry, argmax index].  Predictions are ordered by descending
 *   confidence with ties in row order (a stable sort; the reference's np.argsort(-conf) leaves ties unordered).
 *   ws: scratch of at least sodt_ap_per_class_workspace_bytes(n, nt, nc).
 * sodt_confusion_update: ConfusionMatrix.process_batch (metrics.py:117-155) for every image of a batch at once.
 *   det / det_off / targets / geom as sodt_eval_match.  geom may be NULL: the boxes are then taken as they are and
 *   targets rows are [img cls x1 y1 x2 y2] (process_batch's own arguments, already in native pixels).  nc <= 4096;
 *   conf / iou_thres: host floats, both compared strictly (conf > conf, iou > iou_thres).
 *   matrix: device int64[(nc+1)*(nc+1)], row-major, ADDED into.  Per image, box_iou(labels, detections) of the kept
 *   detections bit for bit as above; every detection keeps its highest-IoU pair, then every label its highest-IoU pair
 *   among those (equal IoU: the lower label index, then the lower detection index; unspecified in the reference).
 *   A label with a pair counts at [gt class, detection class], any other label at [nc, gt class]; a kept detection
 *   without a surviving pair counts at [detection class, nc] only when the image has at least one pair (metrics.py:152).
 *   Pair indices are int32 (the reference's int16 wraps above 32767 rows per image).  info: device int32[2], ADDED
 *   into: [labels, kept detections] whose class is not an integral value in [0, nc); a count that needs such a class
 *   is not written.  ws: scratch of at least sodt_confusion_update_workspace_bytes(B, n_det, nt).
 * No entry allocates or synchronises. */
int sodt_eval_match_workspace_bytes(int B, long n_det, long nt, size_t* bytes);
int sodt_eval_match(const float* det, const int* det_off, int B, long n_det, const float* targets, long nt,
                    const float* geom, const float* iouv, void* ws, size_t ws_bytes, unsigned char* correct,
                    float* tcls_out, sodt_stream_t st);
int sodt_ap_per_class_workspace_bytes(long n, long nt, int nc, size_t* bytes);
int sodt_ap_per_class(const unsigned char* tp, const float* conf, const float* pred_cls, long n, const float* target_cls,
                      long nt, int nc, void* ws, size_t ws_bytes, double* p, double* r, double* f1, double* ap,
                      int* classes, int* nt_count, int* info, sodt_stream_t st);
int sodt_confusion_update_workspace_bytes(int B, long n_det, long nt, size_t* bytes);
int sodt_confusion_update(const float* det, const int* det_off, int B, long n_det, const float* targets, long nt,
                          const float* geom, int nc, float conf, float iou_thres, void* ws, size_t ws_bytes,
                          long long* matrix, int* info, sodt_stream_t st);

/* Batched parameter preparation: out = cast(permute3(in)) for a device-resident table. */
typedef struct {
  const float* src; void* dst;
  int d0, d1, d2;       /* source viewed as [d0][d1][d2] */
  int p0, p1, p2;       /* destination dims order: dst[i_p0][i_p1][i_p2] */
  int dst_ld;           /* elements per destination "row" (>= product of the trailing two dims) */
  int inner_ld;         /* elements between consecutive i_p1 (0: the extent of dims[p2], i.e. dense) - > extent when dims[p2] is zero-padded */
} sodt_prep_desc;
int sodt_prep_weights(const sodt_prep_desc* table_dev, int n, int max_elems, int dtype, sodt_stream_t st);

/* Fused optimizer step over the flat f32 parameter / gradient / momentum / EMA buffers (csrc/optim.hip): what the reference
 * does with torch.optim.SGD(momentum, nesterov) over the weight-decay groups of basics/optimizer.py:35-49 (Train.py:145-150,
 * :448-450), ModelEMA.update (basics/utils/torch_utils.py:291-301) and the cast of the masters to the run dtype, in one
 * streaming launch.  All buffers hold n_elems f32 (16-byte aligned, n_elems % 4 == 0); every 4-element chunk belongs to
 * one parameter and group_of_chunk[chunk] (device bytes, nullable = all group 0) picks its hyper-parameters
 * lr / momentum / weight_decay[group] (host arrays of ngroups <= 4); 255 = not trained (cast / EMA only).
 * Map bytes the call's groups do not name: a byte in [ngroups, 4) is trained with group 0's hyper-parameters (the unused slots
 * of the 4-entry tables repeat slot 0); every byte from 4 to 254 is what 255 is.  A chunk that is not trained keeps its p and
 * momentum bits and still gets the EMA and the cast of its unchanged p (unlike sodt_sam_perturb, which writes nothing there).
 *   d = g*grad_scale + wd*p;  m = momentum*m + d;  u = nesterov ? d + momentum*m : m;  p -= lr*u
 *   ema = ema*ema_decay + (1-ema_decay)*p (ema nullable);  p_cast = (cast_dtype) p (p_cast nullable). */
int sodt_sgd_ema_step(float* p, const float* g, float* mom, float* ema, void* p_cast, int cast_dtype,
                      const unsigned char* group_of_chunk, long n_elems, int ngroups, const float* lr,
                      const float* momentum, const float* weight_decay, int nesterov, float grad_scale,
                      float ema_decay, sodt_stream_t st);

/* The Adam sibling of sodt_sgd_ema_step (csrc/optim.hip), same buffers, group map, EMA and cast tail, one launch: what the
 * reference does with optim.Adam(pg0, lr=hyp['lr0'], betas=(hyp['momentum'], 0.999)) under --adam (Train.py:147-148, :627)
 * over the same weight-decay groups, or with the AdamW of basics/optimizer.py:11-33 (decoupled != 0), followed by
 * ModelEMA.update and the cast.  torch.optim.Adam / AdamW semantics with amsgrad=False, maximize=False; step = t >= 1 is
 * the number of this update (one counter: every owned parameter steps together).  lr / beta1 / beta2 / eps / weight_decay
 * are host arrays of ngroups <= 4 DOUBLES: 1 - beta, lr / (1 - beta1^t), sqrt(1 - beta2^t) and 1 - lr*wd are formed from
 * them in double, as torch forms them from Python floats, and only then rounded to the floats the kernel reads.
 *   coupled: d = g*grad_scale + wd*p, p0 = p;   decoupled: d = g*grad_scale, p0 = p*(1 - lr*wd)
 *   m = b1*m + (1-b1)*d;  v = b2*v + (1-b2)*d*d;  p = p0 - lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 *   ema, p_cast and the map bytes ([ngroups, 4): group 0's hyper-parameters; 4..254: as 255, exp_avg and exp_avg_sq kept too)
 *   as in sodt_sgd_ema_step.  SODT_EINVAL: null / misaligned buffers, n_elems % 4, ngroups outside 1..4,
 *   step < 1, eps <= 0, a beta outside [0, 1), an unknown cast_dtype. */
int sodt_adam_ema_step(float* p, const float* g, float* exp_avg, float* exp_avg_sq, float* ema, void* p_cast, int cast_dtype,
                       const unsigned char* group_of_chunk, long n_elems, int ngroups, const double* lr,
                       const double* beta1, const double* beta2, const double* eps, const double* weight_decay,
                       int decoupled, long step, float grad_scale, float ema_decay, sodt_stream_t st);

/* The control path of the two fused steps (csrc/optim.hip): torch.amp.GradScaler (Train.py:285, :445-450: scaler.step(optimizer),
 * scaler.update()), a skipped step when a gradient is not finite, and global-norm clipping (torch.nn.utils.clip_grad_norm_),
 * with every decision taken on the device so that the host never waits.  sodt_grad_stats fills a 64-byte record in device
 * memory (16-byte aligned) and the _ctl steps read it:
 *   offset  0  double    acc_sumsq      work words of sodt_grad_stats: the entry zeroes these 16 bytes before its launch,
 *           8  unsigned  acc_found      blocks touch them with device-scope atomics only
 *          12  unsigned  ticket
 *          16  double    sumsq          sum of squares of the owned gradient as stored (still scaled), accumulated in f64
 *          24  double    grad_norm      sqrt(sumsq) * |grad_scale / scale|: the norm of the gradient the update sees, unclipped
 *          32  long long step           applied updates so far; sodt_grad_stats adds 1 unless it sets skip.  The caller
 *                                       initialises it (0 for a new optimizer) and may rewrite it between calls (resume)
 *          40  float     found_inf      1 if an owned gradient element is inf / NaN or *found_inf_in != 0, else 0
 *          44  float     inv_scale_eff  (float)(grad_scale / scale * clip_coef): what the step multiplies the gradient by
 *          48  float     clip_coef      max_norm > 0: min(1, max_norm / (grad_norm + 1e-6)); else 1
 *          52  int       skip           found_inf && skip_nonfinite
 *          56  int       reserved[2] */
typedef struct {
  double acc_sumsq; unsigned acc_found, ticket;
  double sumsq, grad_norm; long long step;
  float found_inf, inv_scale_eff, clip_coef; int skip; int reserved[2];
} sodt_step_ctl;

/* One pass over g (n_elems f32, 16-byte aligned, n_elems % 4 == 0; group_of_chunk as in sodt_sgd_ema_step: chunks marked 255 are
 * not owned and never looked at; the entry takes no ngroups: every byte below 4 is owned and every byte from 4 to 254 is what 255
 * is, exactly the chunks the step entries train); the last block to finish finalises *ctl.  scale and found_inf_in are DEVICE pointers to one f32 each
 * (GradScaler's own tensors), either may be null: scale null = 1, 1 / scale is formed as GradScaler forms it
 * (double reciprocal rounded to f32); found_inf_in is OR-ed into found_inf.  grad_scale is the host factor of the plain
 * entries and composes by multiplication.  max_norm <= 0: no clipping.  SODT_EINVAL: null / misaligned g or ctl (16 bytes),
 * misaligned scale / found_inf_in (4 bytes), n_elems % 4, a NaN grad_scale or max_norm. */
int sodt_grad_stats(const float* g, const unsigned char* group_of_chunk, long n_elems, const float* scale,
                    const float* found_inf_in, float grad_scale, float max_norm, int skip_nonfinite, sodt_step_ctl* ctl,
                    sodt_stream_t st);

/* sodt_sgd_ema_step / sodt_adam_ema_step with grad_scale replaced by ctl->inv_scale_eff and, for Adam, step by ctl->step
 * (lr / (1 - beta1^t) and sqrt(1 - beta2^t) are then formed in the kernel, in double from the double hyper-parameters).
 * ctl->skip != 0: p, the momentum / exp_avg / exp_avg_sq are left as they are, while the EMA average and the run-dtype cast
 * still run on the unchanged p (Train.py:450-453 calls ema.update after a skipped step too).  ctl is a DEVICE pointer that a
 * sodt_grad_stats call earlier on the same stream has filled.  Map bytes as in the plain entries: below 4 trained ([ngroups, 4)
 * with group 0's hyper-parameters), 4..254 as 255.  SODT_EINVAL additionally: a null or misaligned (16 bytes) ctl. */
int sodt_sgd_ema_step_ctl(float* p, const float* g, float* mom, float* ema, void* p_cast, int cast_dtype,
                          const unsigned char* group_of_chunk, long n_elems, int ngroups, const float* lr,
                          const float* momentum, const float* weight_decay, int nesterov, const sodt_step_ctl* ctl,
                          float ema_decay, sodt_stream_t st);
int sodt_adam_ema_step_ctl(float* p, const float* g, float* exp_avg, float* exp_avg_sq, float* ema, void* p_cast, int cast_dtype,
                           const unsigned char* group_of_chunk, long n_elems, int ngroups, const double* lr,
                           const double* beta1, const double* beta2, const double* eps, const double* weight_decay,
                           int decoupled, const sodt_step_ctl* ctl, float ema_decay, sodt_stream_t st);

/* Sharpness-aware minimisation around the fused steps (csrc/sam.hip): basics/utils/sam.py over the same flat f32 buffers and
 * the same group_of_chunk map (4-element chunks, ngroups <= 4, chunks marked 255 are not owned: never measured, never
 * written, in p, old_p and the mirror alike).  rho (floats) and adaptive (ints, non-zero = set) are host arrays of ngroups.
 * A map byte in [ngroups, 4) names no group of the call: its chunk enters the norm unweighted and is perturbed with rho 0, that
 * is, left where it is (old_p and the mirror are still written for it).
 * The three entries share a 64-byte record in device memory (16-byte aligned), passed as a double* because it is eight
 * 8-byte words; no C type is declared for it:
 *   offset  0  double    acc_sumsq   work words of sodt_sam_norm: the entry zeroes these 16 bytes before its launch,
 *           8  unsigned  acc_found   blocks touch them with device-scope atomics only
 *          12  unsigned  ticket
 *          16  double    sumsq       sum over the owned elements of (w * g)^2, g as stored (still scaled), accumulated in f64
 *          24  double    norm        sqrt(sumsq) * |inv_scale|: the norm sam.py:49-59 forms, of the unscaled gradient
 *          32  double    inv         found ? 0 : 1 / (norm + 1e-12)      (sam.py:18: rho / (grad_norm + 1e-12), without rho)
 *          40  float     found       1 if an owned gradient element is inf / NaN or the norm is not finite, else 0
 *          44  float     inv_scale   (float)(grad_scale / scale): what the perturbation multiplies the stored gradient by
 *          48  int       reserved[4] */

/* sam.py:49-59 (SAM._grad_norm: one norm per tensor, stacked, and a norm of those) in one pass: w = |p| for a group whose
 * adaptive flag is set, else 1; the last block to finish finalises *rec.  p is read only if some group is adaptive and may be
 * null otherwise.  scale is a DEVICE pointer to one f32 (GradScaler's scale tensor) or null = 1; 1 / scale is formed as in
 * sodt_grad_stats and grad_scale, the host factor, composes by multiplication.  SODT_EINVAL (nothing is touched): null or
 * misaligned (16 bytes) g or rec, a misaligned p, p null with an adaptive group, null adaptive, misaligned scale (4 bytes),
 * n_elems % 4, ngroups outside 1..4, a NaN grad_scale. */
int sodt_sam_norm(const float* p, const float* g, const unsigned char* group_of_chunk, long n_elems, int ngroups,
                  const int* adaptive, const float* scale, float grad_scale, double* rec, sodt_stream_t st);

/* sam.py:19-25 (SAM.first_step's loop: old_p = p.data.clone(); e_w = (p^2 if adaptive else 1) * p.grad * scale; p.add_(e_w))
 * in one pass over the owned chunks:
 *   old_p = p;   p += (adaptive ? p*p : 1) * g * rec.inv_scale * (rho[group] * rec.inv);   p_cast = (cast_dtype) p
 * rec is a DEVICE pointer that a sodt_sam_norm call earlier on the same stream has filled.  p_cast (the run-dtype mirror) is
 * nullable.  With rec.found set, p stays bit for bit what it was; old_p = p and the cast are still written.  SODT_EINVAL
 * (nothing is touched): null or misaligned (16 bytes) p, g, old_p or rec, a misaligned p_cast, n_elems % 4, ngroups outside
 * 1..4, null rho / adaptive, a negative or NaN rho, an unknown cast_dtype. */
int sodt_sam_perturb(float* p, const float* g, float* old_p, void* p_cast, int cast_dtype, const unsigned char* group_of_chunk,
                     long n_elems, int ngroups, const float* rho, const int* adaptive, const double* rec, sodt_stream_t st);

/* sam.py:30-34 (SAM.second_step's loop: p.data = old_p) as a copy into the flat buffer, owned chunks only; the step that
 * follows rewrites the mirror.  SODT_EINVAL: null or misaligned (16 bytes) p or old_p, n_elems % 4. */
int sodt_sam_restore(float* p, const float* old_p, const unsigned char* group_of_chunk, long n_elems, sodt_stream_t st);

/* Input pre-processing of the training / evaluation loop (csrc/preprocess.hip): `imgs.to(device).float() / 255.0` followed by
 * `F.interpolate(image, size=[i // down_factor ...], mode='bilinear', align_corners=True)` (Train.py:364-374; test.py:124-129
 * is the factor-1 case) for the RGB and the IR batch in one launch.  rgb / ir: uint8 (B, c, Hin, Win) contiguous (device);
 * out_rgb / out_ir: f32 (B, c, Hout, Wout), the planes sodt_frontend_fwd reads.  Hout <= Hin, Wout <= Win; Hout == Hin is
 * the plain u8 -> f32 / 255.  c_ir may be 0 (ir, out_ir then unused). */
int sodt_preprocess_u8(const unsigned char* rgb, const unsigned char* ir, float* out_rgb, float* out_ir, int B, int c_rgb,
                       int c_ir, int Hin, int Win, int Hout, int Wout, sodt_stream_t st);

/* Multi-scale training (csrc/multiscale.hip): the pre-processing above followed by the resize of `--multi-scale`,
 * `F.interpolate(imgs, size=ns, mode='bilinear', align_corners=False)` (Train.py:396-402), for the RGB and the IR batch in
 * one launch with no global intermediate and no workspace.  rgb / ir: uint8 (B, c, Hin, Win) contiguous (device); the
 * align-corners shrink goes to (Hmid, Wmid) (Hmid <= Hin, Wmid <= Win; Hmid == Hin: no shrink), the half-pixel resize from there
 * to (Hout, Wout), larger or smaller; out_rgb / out_ir: f32 (B, c, Hout, Wout).  Each stage takes its source index and blend
 * weight from an exact integer quotient and remainder, and the stage-1 values are rounded to f32 as the reference's
 * intermediate tensor is.  SODT_EINVAL, nothing written: a null pointer, a non-positive size or channel count, Hmid > Hin or
 * Wmid > Win, or one of Hin * Hmid, Win * Wmid, 2 * Hout * Hmid, 2 * Wout * Wmid, Hin * Win reaching 2^31. */
int sodt_preprocess_u8_ms(const unsigned char* rgb, const unsigned char* ir, float* out_rgb, float* out_ir, int B, int c_rgb,
                          int c_ir, int Hin, int Win, int Hmid, int Wmid, int Hout, int Wout, sodt_stream_t st);

/* Quad collate (csrc/quad.hip): the image side of LoadImagesAndLabels.collate_fn4 (basics/utils/datasets.py:637-664, the
 * loader of `--quad`, Train.py:223).  rgb / ir: uint8 (B, c, H, W) contiguous (device), the SOURCE batch; n = B / 4 groups
 * of four consecutive samples, samples 4n .. B-1 unused.  Bit g of zoom_mask is the draw of group g (datasets.py:647): set,
 * the group's image is sample 4g zoomed 2x as `F.interpolate(..., scale_factor=2., mode='bilinear', align_corners=False)`
 * cast back to uint8 does (datasets.py:648-651), evaluated as the integer expression (9 a + 3 b + 3 c + d) >> 4 that call
 * equals byte for byte; clear, the four samples tiled 2 x 2, sample 4g+1 BELOW 4g and 4g+2 to its RIGHT (datasets.py:654-655).
 * The mask travels by value: no device table, no copy, at most 64 groups.  c_ir may be 0 (ir, out_ir then unused).
 *
 * sodt_quad_u8 replaces the image outputs of collate_fn4 themselves: out_rgb / out_ir uint8 (n, c, 2H, 2W), what SRLoss
 * reads under `--super` and what sodt_preprocess_u8_ms resizes under `--multi-scale`.
 * sodt_preprocess_u8_quad replaces collate_fn4 AND the pre-processing of Train.py:364-374 after it (sodt_preprocess_u8 on the
 * quad batch, same arithmetic, same bits) in one launch from the source batch, with no uint8 intermediate: out_rgb / out_ir
 * f32 (n, c, Hout, Wout), Hout <= 2H, Wout <= 2W.
 * SODT_EINVAL, nothing written: a null pointer, B < 4, B / 4 > 64, a non-positive size or channel count (c_ir < 0), Hout > 2H
 * or Wout > 2W, or one of 4 * H * W, 2H * Hout, 2W * Wout reaching 2^31. */
int sodt_quad_u8(const unsigned char* rgb, const unsigned char* ir, unsigned char* out_rgb, unsigned char* out_ir, int B,
                 int c_rgb, int c_ir, int H, int W, unsigned long long zoom_mask, sodt_stream_t st);
int sodt_preprocess_u8_quad(const unsigned char* rgb, const unsigned char* ir, float* out_rgb, float* out_ir, int B, int c_rgb,
                            int c_ir, int H, int W, int Hout, int Wout, unsigned long long zoom_mask, sodt_stream_t st);

/* ComputeLoss.__call__ + build_targets (basics/utils/loss.py:116-224) with bbox_iou(CIoU) (basics/utils/general.py:347-389)
 * for the single detection layer of models/model.yaml: loss values and d(loss * batch) / d pred in one call.
 * pred f32 (B, na, ny, nx, 5+nc) contiguous; targets f32 (nt, 6) = (image, class, x, y, w, h) normalised (device);
 * anchors f32 (na, 2) in grid units (Detect.anchors[0]); hyper-parameters as in models/hyp.scratch.yaml (box, cls,
 * cls_pw, obj, obj_pw, anchor_t) and model.gr.  dpred f32 like pred; out4 = (loss * B, lbox, lobj, lcls) as loss.py:163.
 * Duplicate cells take the objectness target of the LAST matching candidate in the reference's order (CPU index_put).
 * Rows whose image index is outside [0, B) are skipped: the kernel skips such rows where the reference would raise.
 * ws: scratch of sodt_yolo_loss_workspace_bytes(B*na*ny*nx, nt, nc) bytes.  nc <= 32, na <= 8. */
int sodt_yolo_loss_workspace_bytes(long ncells, int nt, int nc, size_t* bytes);
int sodt_yolo_loss(const float* pred, const float* targets, int nt, const float* anchors, int B, int na, int ny, int nx,
                   int nc, float h_box, float h_cls, float cls_pw, float h_obj, float obj_pw, float anchor_t, float gr,
                   void* ws, size_t ws_bytes, float* dpred, float* out4, sodt_stream_t st);
/* The same with the reference's FocalLoss(BCEWithLogitsLoss(pos_weight), gamma=fl_gamma, alpha=0.25) around the class and
 * the objectness BCE (basics/utils/loss.py:36-62, :103-108; hyp['fl_gamma'], mutated by --evolve, Train.py:720), value and
 * gradient.  fl_gamma == 0 is sodt_yolo_loss, kernel for kernel; fl_gamma < 0 or NaN: SODT_EINVAL.  The gradient stays
 * finite where 1 - p_t rounds to 0 (saturated logits, gamma < 1), where the reference's autograd gives inf * 0. */
int sodt_yolo_loss_fl(const float* pred, const float* targets, int nt, const float* anchors, int B, int na, int ny, int nx,
                      int nc, float h_box, float h_cls, float cls_pw, float h_obj, float obj_pw, float anchor_t, float gr,
                      float fl_gamma, void* ws, size_t ws_bytes, float* dpred, float* out4, sodt_stream_t st);

/* The super-resolution term of the training loss under --super (csrc/srloss.hip), Train.py:420-427:
 *   SODT_SR_IR      0.5 * L1Loss()(output_sr, ir_image)                                      C == 1, plane 0 of ir
 *   SODT_SR_RGB     0.5 * L1Loss()(output_sr, image)                                         C == c_rgb
 *   SODT_SR_RGB_IR  0.1 * (L1Loss()(output_sr[:, 0:3], image) + L1Loss()(output_sr[:, 3:], ir_image[:, 0:1]))
 *                                                                                            C == 4, c_rgb == 3
 * with image = imgs.float() / 255.0 (Train.py:364-365) formed per element from the uint8 batch, never stored.
 * sr: output_sr, f32 (B, C, H, W) contiguous.  rgb / ir: (B, c_rgb, H, W) / (B, c_ir, H, W) contiguous, target_dtype SODT_U8
 * (the dataloader's batches; t = float(u8) / 255.0f, bit for bit torch's) or SODT_F32 (targets already in [0, 1]); of ir
 * (c_ir >= 1) only plane 0 of each image is read; the tensor a mode does not use may be NULL.  B * C <= 65535, H * W < 2^31.
 * sodt_sr_l1_fwd: one pass; |o - t| in f32, the sums of the two groups (planes 0:3, plane 3; one group in the one-mode
 *   branches) in f64 through per-block partials in ws that the last block (a ticket) adds in block order: *loss (device,
 *   one f32) = (float)(w * (s0 / n0 + s1 / n1)), the same bits for the same inputs on every call.  ws: 16-byte aligned,
 *   at least sodt_sr_l1_workspace_bytes(B, C, H, W); its first 16 bytes are zeroed by the entry before the launch.
 * sodt_sr_l1_bwd: one pass; dsr (f32, like sr) = (float)(*upstream * w / n_group) * sign(o - t), sign(0) = 0, from sr and the
 *   targets again (nothing is kept from the forward).  upstream: DEVICE pointer to one f32, the incoming gradient of the loss
 *   (GradScaler's scale, the world size and the --quad factor of Train.py:439-445 arrive through it).
 * Planes whose size is not a multiple of 4, or unaligned bases, run the element-wise form of the same kernels.
 * SODT_EINVAL, nothing launched or written: a null pointer that the mode needs, a shape outside the above, C / c_rgb / c_ir
 * that do not fit the mode, an unknown mode or target_dtype, f32 pointers off a 4-byte boundary, ws too small or unaligned. */
#define SODT_U8 2
#define SODT_SR_IR 0
#define SODT_SR_RGB 1
#define SODT_SR_RGB_IR 2
int sodt_sr_l1_workspace_bytes(int B, int C, int H, int W, size_t* bytes);
int sodt_sr_l1_fwd(const float* sr, const void* rgb, const void* ir, int target_dtype, int mode, int B, int C, int c_rgb,
                   int c_ir, int H, int W, void* ws, size_t ws_bytes, float* loss, sodt_stream_t st);
int sodt_sr_l1_bwd(const float* sr, const void* rgb, const void* ir, int target_dtype, int mode, int B, int C, int c_rgb,
                   int c_ir, int H, int W, const float* upstream, float* dsr, sodt_stream_t st);

/* ---- autoanchor (basics/utils/autoanchor.py: check_anchors :24-60, kmean_anchors :63-158), start-up only (csrc/autoanchor.hip) ----
 * wh: (N, 2) f32 label sizes in pixels (8-byte aligned), finite and positive.  An anchor set is (n, 2) f32, 1 <= n <= 32.
 * The ratio metric of :33-35 / :80-84 per label, in f32 with IEEE division: r = wh / k, x = min over the two axes of
 * min(r, 1 / r), best = max over the anchors of x.  thr is the threshold ALREADY inverted (1 / anchor_t) and rounded to
 * f32, compared strictly in f32 - the rule of torch's `float32_tensor > python_float`.  Sums are f64 and counts int64,
 * reduced per block and added by the last block in block order: equal inputs give equal bits on every call.
 * sodt_anchor_stats: `metric` (:33-39, :80-84), `anchor_fitness` (:86-88) and every figure of `print_results` (:90-96) for
 *   S anchor sets (S, n, 2) at once.  out: (S, 6) f64 per set: sum(best), sum(best [best > thr]), count(best > thr),
 *   count(x > thr) over all N * n, sum(x), sum(x [x > thr]).  bpr = out[2] / N, aat = out[3] / N, fitness = out[1] / N.
 *   N == 0 writes zeros.  S <= 65535.  ws: 16-byte aligned, at least sodt_anchor_stats_workspace_bytes(N, S).
 * sodt_anchor_evolve: the G generations of :146-153 without a host read.  k: (n, 2) f64 and f: one f64, both DEVICE, in
 *   and out; v: (G, n, 2) f64 DEVICE, the mutation factors of :147-149 (they depend on the random stream only).  For
 *   g = 0 .. G-1 in order, one launch each: kg = max(k * v[g], 2.0) in f64; fg = sum(best [best > thr]) / N of float32(kg),
 *   the sum and the mean in f64; if fg > f (f64) then f, k = fg, kg.  accepted: nullable (G) int32, 1 where generation g
 *   was taken.  G == 0 launches nothing.  N >= 1.  ws: at least sodt_anchor_evolve_workspace_bytes(N).
 * sodt_kmeans_lloyd: `iters` iterations of the loop inside scipy.cluster.vq.kmeans (:123) for R restarts at once, all in
 *   f64.  obs: (N, 2) whitened points (16-byte aligned), N >= 1.  books: (R, n, 2), in and out; alive: (R, n) int32, 1 = the
 *   centre is live; prev: (R) the last mean distortion (the caller starts it at +inf); done: (R) int32.  One iteration of a
 *   restart that is not done: every point goes to its nearest live centre by dx*dx + dy*dy (not contracted; ties to the
 *   lowest live index), cur = mean of the square roots, every live centre moves to the mean of its members, one without
 *   members is marked dead (its book row is left as it is and its slot kept, so the order of the others stays),
 *   diff = |prev - cur|, prev = cur, done = diff <= thresh - so the book is moved once more after the last distortion,
 *   as scipy does.  A restart whose done is set is not touched again.  R <= 65535.
 *   ws: at least sodt_kmeans_lloyd_workspace_bytes(N, R, n).
 * SODT_EINVAL, nothing launched or written: n outside 1..32, a null or misaligned pointer, N / S / R / G / iters outside the
 * above, a NaN threshold, ws too small.  No entry allocates or synchronises. */
int sodt_anchor_stats_workspace_bytes(long N, int S, size_t* bytes);
int sodt_anchor_stats(const float* wh, long N, const float* sets, int S, int n, float thr, void* ws, size_t ws_bytes,
                      double* out, sodt_stream_t st);
int sodt_anchor_evolve_workspace_bytes(long N, size_t* bytes);
int sodt_anchor_evolve(const float* wh, long N, float thr, double* k, int n, double* f, const double* v, int G,
                       int* accepted, void* ws, size_t ws_bytes, sodt_stream_t st);
int sodt_kmeans_lloyd_workspace_bytes(long N, int R, int n, size_t* bytes);
int sodt_kmeans_lloyd(const double* obs, long N, double* books, int* alive, double* prev, int* done, int R, int n,
                      double thresh, int iters, void* ws, size_t ws_bytes, sodt_stream_t st);

/* ---- --image-weights (Train.py:335-341; basics/utils/general.py: labels_to_class_weights :220-236, labels_to_image_weights
 *      :239-244; random.choices), once per epoch (csrc/sampling.hip) ----
 * status: one int32 on the device that the entries OR the SODT_SAMPLING_* bits into; the caller zeroes it.
 * sodt_class_counts: the np.bincount of :227 and :241 for all images at once.  cls, img: (M) int32, the class and the image
 *   id of every label.  One thread per label (a grid-stride loop beyond 262,144 labels) adds 1 to counts[img][cls], (n_img, nc)
 *   int32, and to class_total[cls], (nc) int64, with integer atomics - exact in any order; the caller zeroes both.  Up to
 *   nc = 1024 a block gathers its class totals in LDS and adds each once; above that every label adds to class_total.  A class
 *   outside [0, nc) or an image id outside [0, n_img) sets its status bit and is not counted.  M == 0 launches nothing.
 *   0 <= M < 2^31, 1 <= n_img <= 2^24, 1 <= nc <= 65536.
 * sodt_image_weights: iw[i] = sum over c of cw[c] * counts[i][c] (:242), f64: ONE accumulator per image that starts at +0.0
 *   and takes the classes in ascending order, each product rounded before it is added (no fused multiply-add, no atomics).
 *   Rows of `counts` are read as runs of up to 32 classes through LDS.
 * sodt_weighted_choices: `random.choices(range(n), weights=iw, k=k)` from k uniform numbers u (k) f64 in [0, 1), the values
 *   random.random() returned in draw order.  cum: (n) f64, an output (it may follow the workspace in one allocation): the
 *   inclusive prefix sums of iw.  Their association order depends on n alone and no atomic is used, so equal inputs give
 *   equal bits on every call.  With W = SODT_CHOICES_BLOCK = 1024 and iw padded with +0.0 to a multiple of W:
 *     phase 1, one block of 256 threads per W weights: thread t takes the 4 consecutive weights a0..a3 from 4 t,
 *       s0 = a0, s_j = s_(j-1) + a_j.  The 256 thread sums s3 are scanned (`block scan`): within each wave of 64 lanes
 *       by Hillis-Steele, v[l] = v[l] + v[l - o] for all l >= o at once, o = 1, 2, 4, 8, 16, 32; the wave sums W0..W3 (lane 63)
 *       give the wave prefixes 0.0, W0, W0 + W1, (W0 + W1) + W2 and the block sum ((W0 + W1) + W2) + W3; the exclusive prefix of
 *       thread t is wave_prefix + (lane > 0 ? v[lane - 1] : 0.0).  local[4 t + j] = prefix_t + s_j.
 *     phase 2, ONE block: the nb = ceil(n / W) block sums, padded with +0.0 to 256 * per, per = ceil(nb / 256); thread t takes
 *       the `per` consecutive sums from t * per serially as above, the thread sums go through the same block scan, and
 *       inclusive[t * per + j] = prefix_t + s_j.  offset[0] = 0.0, offset[b + 1] = inclusive[b].
 *     phase 3: cum[e] = offset[e / W] + local[e].
 *   total = cum[n - 1].  total <= 0: SODT_SAMPLING_ZERO_TOTAL; otherwise total NaN or infinite: SODT_SAMPLING_NONFINITE_TOTAL;
 *   in both cases every idx is -1.  Otherwise draw j forms x = u[j] * total (one IEEE multiply) and idx[j] = the number of
 *   entries of cum[0 .. n-2] that are <= x, i.e. Python's bisect_right(cum, x, 0, n - 1): an x that equals a boundary goes
 *   right, an image of weight zero is never drawn, and the result is at most n - 1.  idx: (k) int32.  1 <= n <= 2^24,
 *   0 <= k <= 2^24.  ws: 16-byte aligned, at least sodt_weighted_choices_workspace_bytes(n, k).
 * SODT_EINVAL, nothing launched or written: a null or misaligned pointer (4 bytes for int32, 8 for int64 and f64, 16 for ws),
 * a size outside the above, ws too small.  No entry allocates, synchronises or reads the environment. */
#define SODT_CHOICES_BLOCK 1024
#define SODT_SAMPLING_BAD_CLASS 1
#define SODT_SAMPLING_BAD_IMAGE 2
#define SODT_SAMPLING_ZERO_TOTAL 4
#define SODT_SAMPLING_NONFINITE_TOTAL 8
int sodt_class_counts(const int* cls, const int* img, long M, int n_img, int nc, int* counts, long long* class_total,
                      int* status, sodt_stream_t st);
int sodt_image_weights(const int* counts, const double* cw, int n_img, int nc, double* iw, sodt_stream_t st);
int sodt_weighted_choices_workspace_bytes(int n, int k, size_t* bytes);
int sodt_weighted_choices(const double* iw, int n, const double* u, int k, int* idx, double* cum, int* status, void* ws,
                          size_t ws_bytes, sodt_stream_t st);

/* hipMemsetAsync(p, 0, bytes) on the stream (statistics / gradient accumulators) */
int sodt_memset_zero(void* p, long bytes, sodt_stream_t st);

/* bias table (L, heads) f32 -> (heads, L) f32, and the reverse accumulate for its gradient
 * (accumulate: 0 = store, 1 = add, 2 = add and clear the source) */
int sodt_transpose_f32(const float* src, float* dst, int rows, int cols, int accumulate, sodt_stream_t st);

/* out[r][c] (f32) += sum_b d[b][r][c]: gradient of the batch-broadcast pos_embed add (backbone_vit.py:215-217) */
int sodt_batch_sum(const void* d, float* out, int B, long RC, int dtype, sodt_stream_t st);

/* f32 <-> run dtype elementwise cast */
int sodt_cast(const void* src, void* dst, long n, int src_dtype, int dst_dtype, sodt_stream_t st);

const char* sodt_version(void);

#ifdef __cplusplus
}
#endif
#endif

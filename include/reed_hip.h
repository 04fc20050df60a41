/*
 * reed_hip.h — C ABI of libreed_hip.so, the MI355X (gfx950) kernel library behind the
 * reed_amd drop-in for REED's image/ SiT training + sampling path.
 *
 * The reference (ChenyuWang-Monica/REED, image/) has no FFI of its own: it is pure PyTorch.
 * Each entry point below replaces the arithmetic of the reference lines cited next to it; the
 * Python host (reed_amd/) binds them with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (PyTorch allocates; the library never
 *    allocates, frees or retains memory past the call); tensors are contiguous row-major unless
 *    a leading dimension argument says otherwise;
 *  - `stream` is a hipStream_t passed as void* (PyTorch's current stream); all work is enqueued
 *    there and the call returns immediately;
 *  - return value 0 = OK, otherwise an argument-check code (1001/1002) or a hipError_t;
 *    reed_last_error() returns a thread-local message;
 *  - dtypes are fixed per entry point: "bf16" = __bf16 / torch.bfloat16, f32, f64, i64.
 */
#ifndef REED_HIP_H
#define REED_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

const char* reed_last_error(void);
int reed_version(void);
/* 0: this library was built with bfloat16 operands (libreed_hip.so: the training path); 1: IEEE half operands
 * (libreed_hip_f16.so, the same sources with -DREED_FP16: the sampling path at the mantissa of the reference's TF32) */
int reed_half_kind(void);

/* ---------------------------------------------------------------------------------------------
 * Dense contractions (every nn.Linear on the path: sit.py:17-24 projector, :38-42 t-MLP,
 * :114-124 attention qkv/proj + Mlp fc1/fc2 (timm), :126-129 & :146-150 adaLN; and their autograd).
 *   layout 0 NT: C[M,N] = P[M,K] Q[N,K]^T     (forward  y = x W^T)
 *   layout 1 NN: C[M,N] = P[M,K] Q[K,N]       (dgrad    dx = dy W)
 *   layout 2 TN: C[M,N] = P[K,M]^T Q[K,N]     (wgrad    dW = dy^T x), optional dbias[M] = colsum(P)
 *   layout 3 / 4: TN on a 256x128 / 128x256 output tile (128x64 / 64x128 per wave; epilogue 6 only; 4 needs N%256==0)
 * epilogue codes: see reed_amd/csrc/gemm.h (11 = exact GELU(erf) with the layout of 9; 0 bf16, 1 gelu, 2 silu, 3 gate+residual, 4 dgelu,
 *   5 dsilu, 6 f32 (+=), 7 f32 += bf16-rounded, 8 f32 atomic, 9 QuickGELU, 10 + bf16 residual, 12 LayerScale + fp32 residual:
 *   C f32 = R f32 + gamma[n] * float(bf16(acc + bias)) with `gate` = the fp32 gamma vector, NT only; 13 = 0 plus the per-row,
 *   per-head partial dot products with R for reed_attention_bwd_dp (NN; returns 1002 without launching where the shape's
 *   kernel has no such epilogue); 14 / 15 = 1 / 2 with C = the activation's DERIVATIVE at the pre-activation instead of the
 *   pre-activation itself (what the backward needs: nothing else read the saved pre-activation), 16 = C bf16 =
 *   bf16(bf16(acc) * R): the activation backward as one multiply by that saved derivative; 17 = SwiGLU (DINOv2 ViT-g's
 *   feed-forward, inference only): C bf16 [M, N/2] (ldc >= N/2) = bf16(float(bf16(silu(x1))) * x2) with x1 | x2 =
 *   bf16(acc + bias), which is never stored.  NT only, no split-K, and Q / bias are PACKED: with g = 8, packed row 2gk + j is
 *   row gk + j of the [N, K] weight (x1) and packed row 2gk + g + j its row N/2 + gk + j (x2), j < g; output column gk + j
 *   (reed_amd/ops.py: swiglu_pack).  The fp32-operand library refuses it (1001).  N%128==0 (NT/NN with a
 *   bf16-output epilogue also N%144==0: the 256x144 tile of csrc/gemm144.hip); K%64==0 (NT/NN);
 *   M%128==0 (TN).  split_k>1 only with epilogue 8, or 6 with slab_stride>0 (C then holds split_k slabs;
 *   dbias likewise holds split_k slabs of M floats AT THE SAME slab_stride — put slab 0 of dbias right behind slab 0
 *   of C and one reed_reduce_slabs call over M*N + M floats finishes both; deterministic).
 * ------------------------------------------------------------------------------------------- */
int reed_gemm(int layout, int epilogue, const void* P, int64_t ldp, const void* Q, int64_t ldq,
              int M, int N, int K, void* C, int64_t ldc, void* C2, int64_t ldc2, const void* R,
              int64_t ldr, const void* bias, const void* gate, int64_t ldgate, int rows_per_gate,
              float* dbias, int accumulate, int split_k, int64_t slab_stride, void* stream);

/* The weight gradients of one transformer block (autograd of the four nn.Linear of image/models/sit.py:114-129's Attention /
 * Mlp) in ONE launch without split-K: n <= 4 problems dw_i f32 [n_out_i, k_in_i] (+)= dy_i[tokens, n_out_i]^T x_i[tokens, k_in_i]
 * (16-bit operands, row-major, leading dims = widths), optional dbias_i f32 [n_out_i] (+)= colsum(dy_i).  Pointer / int
 * arrays live on the host.  k_in % 128 == 0, n_out % 16 == 0.  Returns 1002 without launching when the problems' 256x128 /
 * 128x256 tiles do not fit one round of 2 x CUs workgroups (use reed_gemm layout 3 / 4 with split_k then). */
int reed_wgrad_group(int n, const void* const* dy, const void* const* x, float* const* dw, float* const* dbias,
                     const int* n_out, const int* k_in, int tokens, int accumulate, void* stream);
/* Planning side of reed_wgrad_group (host arithmetic, no device call): how the 16-bit builds' one-workgroup-per-CU form of the
 * grouped launch (csrc/gemm256w.hip: TnGroupW) deals the problems over `cus` CUs.  items[256]: entry x * (cus / 8) + j = the item of
 * workgroup j of XCD x, 0xFFFFFFFF = none; an item = problem | mode << 2 | row unit << 6 | column unit << 14 | (valid row units - 1)
 * << 22 | (valid column units - 1) << 24 | bias gradient << 26 in units of 128 rows / columns of dw: mode 0 = a 256 x 256 tile,
 * 6 = 384 x 128 (+ the bias gradient of its rows), 7 = 128 x 384, 8 = the bias gradient of up to 512 rows, no output.  Returns the
 * number of items; 0 = the form does not apply to these problems (or this build: fp32 operands) and reed_wgrad_group uses the
 * two-workgroups-per-CU kernel (csrc/gemm_tn.hip). */
int reed_wgrad_group_deal(int n, const int* n_out, const int* k_in, const int* has_bias, int cus, unsigned* items);

/* CUs the GEMM tile heuristics plan for: the device's count minus a reserve for kernels that hold CUs
 * beside the GEMMs (RCCL channels during a gradient bucket).  reed_set_cu_reserve(n): n >= 0; reed_planning_cus(): the result. */
int reed_set_cu_reserve(int n);
int reed_planning_cus(void);
/* reed_set_concurrent_comm(1): collectives will run beside the following GEMMs (a data-parallel backward).  Kernels that hold
 * a whole CU per workgroup for their entire run (the persistent form of the 256x256 kernel) are then not selected. */
int reed_set_concurrent_comm(int on);

/* tile selection override for tests / A-B timing: 0 = heuristic (default); 64 (skinny one-wave tiles) / 128 / 144 (256x144) / 256
 * (256x256, eight waves) / 257 (256x256, four waves, one tile per workgroup) / 258 (the same, persistent wherever that form
 * applies) / 288 (256x288) = that kernel wherever the shape allows, the heuristic elsewhere; 259 = heuristic plus the column split */
int reed_gemm_force_tile(int tile);
/* fp32-operand library only: how reed_gemm, reed_conv3x3 and reed_conv3x3_down multiply.  0 (the default) = exact fp32 products on
 * v_mfma_f32_32x32x2_f32; 1 = the reference's --allow-tf32 / generate.py --tf32 on hardware without an xf32 instruction: every fp32
 * operand element x is split into hi = bf16(x) and lo = bf16(x - hi), and a*b is taken as a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on the
 * bf16 MFMA with fp32 accumulation: fp32 operands in memory, fp32's exponent range, an error of at most 3 * 2^-16 of |a||b| per
 * product (TF32 rounding: 2 * 2^-11).  Same shapes, epilogues and arguments either way; the fp32 attention stays exact.  Process-wide;
 * returns 0.  The 16-bit libraries accept 0 and answer 1 with 1002: their operands are 16-bit already. */
int reed_gemm_f32_split(int on);
/* Dry run of reed_gemm's kernel selection (host arithmetic, no device call, no pointers: csrc/gemm_plan.cpp).  layout, epilogue,
 * M, N, K, split_k and rows_per_gate as for reed_gemm; flags: 1 = dbias given, 2 = slab_stride > 0, 4 = R and C2 given.  The knobs
 * are explicit: ncu = CUs to plan for (<= 0: reed_planning_cus()), forced_tile as for reed_gemm_force_tile, colsplit / use288 = the
 * switches REED_GEMM_COLSPLIT / REED_GEMM288 (< 0: as the environment set them at load), concurrent_comm as for
 * reed_set_concurrent_comm.  Returns the number of launches n <= 3 and fills launches[9 n] (NULL: count only) with, per launch,
 * {kernel, row0, rows, col0, cols, splits, ksplit_len, tile_gm, grid}: kernel 0 = 128x128 tiles, 1 = 256x144, 2 = 256x288, 3 = 256x256
 * eight waves, 4 = 256x256 four waves one-shot, 5 = the same persistent, 6 = skinny, 7 = TN 256x128, 8 = TN 128x256, 9 = the
 * fp32-operand library's exact kernel, 10 = its split kernel (that library reports 10 while reed_gemm_f32_split(1) holds, 9
 * otherwise, with the same grid of 128x128 tiles); the launch computes rows [row0, row0 + rows) x columns [col0, col0 + cols) of the output with
 * grid.x = grid, grid.y = splits.  Where reed_gemm would refuse the shape: minus its error code (-1001 / -1002). */
int reed_gemm_plan(int layout, int epilogue, int M, int N, int K, int split_k, int flags, int rows_per_gate, int ncu,
                   int forced_tile, int colsplit, int use288, int concurrent_comm, int* launches);

/* ---------------------------------------------------------------------------------------------
 * MX-fp8 block GEMMs (sampling only; no counterpart in the reference).  Format: OCP e4m3fn elements (bias 7, max 448, NaN 0x7F /
 * 0xFF), blocks of 32 consecutive k, one E8M0 scale byte per block (value 2^(byte - 127)).  Finite block, amax > 0:
 * X = clamp(floor(log2 amax) - 8, -127, 127), byte = X + 127, code = x 2^-X rounded to nearest-even onto the e4m3 grid, signs and
 * subnormals kept, saturated to +-448.  amax = 0: byte 127 and signed zeros.  A block holding an inf or a NaN: byte 0xFF and
 * every code 0x7F; every output that consumes it is NaN.  The fp32-operand library answers all three entries with 1001.
 *
 * reed_mx_quantize: x 16-bit [R, K] (row stride ldx elements) -> codes u8 [R, K] (row stride ldq bytes), scales u8 [R, K/32] (row
 * stride lds bytes).  K % 32 == 0, ldx and ldq multiples of 8, x 16-byte and codes 8-byte aligned.  Writes live elements only.
 * reed_gemm_mxfp8: C[M,N] = epilogue(sum_blocks 2^(Xa + Xw) sum_k a w + bias), fp32 accumulation, NT: Aq [M,K] / Wq [N,K] codes
 * (row strides lda / ldw bytes, multiples of 16) with their scales As [M,K/32] / Ws [N,K/32] (row strides multiples of 4 bytes).
 * Epilogues 0 (bf16), 1 (GELU) and 3 (gate + residual) with reed_gemm's arguments and rounding points.  K % 128 == 0,
 * N % 128 == 0, any M >= 1.
 * reed_gemm_mxfp8_plan: host arithmetic, no device call: 0 where reed_gemm_mxfp8 takes (epilogue, M, N, K), else 1001.
 * ------------------------------------------------------------------------------------------- */
int reed_mx_quantize(const void* x, int64_t ldx, void* codes, int64_t ldq, void* scales, int64_t lds, int R, int K,
                     void* stream);
int reed_gemm_mxfp8(int epilogue, const void* Aq, int64_t lda, const void* As, int64_t ldas, const void* Wq, int64_t ldw,
                    const void* Ws, int64_t ldws, int M, int N, int K, void* C, int64_t ldc, void* C2, int64_t ldc2,
                    const void* R, int64_t ldr, const void* bias, const void* gate, int64_t ldgate, int rows_per_gate,
                    void* stream);
int reed_gemm_mxfp8_plan(int epilogue, int M, int N, int K);

/* bias gradient: out[n] (+)= sum_m x[m,n], x bf16 [M,N] (row stride ld); ws: caller scratch of
 * reed_colsum_ws_floats(M, N) floats. Deterministic (fixed reduction order). */
int64_t reed_colsum_ws_floats(int M, int N);
int reed_colsum_bf16(const void* x, int64_t ld, float* ws, float* out, int M, int N, int accumulate,
                     void* stream);

/* sum split-K slabs: out[i] (+)= sum_z slabs[z*stride + i], i < n */
int reed_reduce_slabs(const float* slabs, int64_t stride, int nslabs, float* out, int64_t n,
                      int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------
 * LayerNorm(eps, no affine) + modulate  (sit.py:26-27,113,119,132-135,143,152)
 *   h[m,:] = bf16( LN(x[m,:]) * bf16(1+scale[b,:]) + shift[b,:] ),  b = m / T
 * x f32 [M,D]; shift/scale bf16 with row stride ldmod; h bf16 [M,D]; mean/rstd f32 [M] (optional).
 * scale==NULL -> plain cast f32->bf16 of x (projector input cast, sit.py:292).
 * mean and rstd are given together or both NULL; one without the other is refused without a launch.
 * ------------------------------------------------------------------------------------------- */
int reed_ln_modulate_fwd(const float* x, const void* shift, const void* scale, int64_t ldmod,
                         void* h, float* mean, float* rstd, int M, int D, int T, float eps,
                         void* stream);
/* backward: dx[m,:] += LNbwd(dh * bf16(1+scale)); partial column sums over each 16-row chunk:
 *   part[(m/16), 0, :] = sum dh, part[(m/16), 1, :] = sum dh*xhat        (f32 [M/16, 2, D]) */
int reed_ln_modulate_bwd(const void* dh, const float* x, const float* mean, const float* rstd,
                         const void* scale, int64_t ldmod, float* dx, float* part, int M, int D,
                         int T, void* stream);

/* the same followed, in the same pass, by the gate backward of the next branch in backward order (the one that
 * consumes the dx just finished): see reed_gate_bwd for dy / part_g / part_dy. Saves one read of the fp32 dx. */
int reed_ln_modulate_bwd_gate(const void* dh, const float* x, const float* mean, const float* rstd,
                              const void* scale, int64_t ldmod, float* dx, float* part, const void* y,
                              const void* gate, int64_t ldgate, void* dy, float* part_g, float* part_dy,
                              int M, int D, int T, void* stream);

/* gate backward (sit.py:134-135): dg = bf16(dx); dy = bf16(dg*gate[b]); part[(m/16),:] = sum bf16(dg*y);
 * optional part_dy[(m/16),:] = sum dy  (bias gradient of the linear that produced y, reduce with reed_rowsum_f32) */
int reed_gate_bwd(const float* dx, const void* y, const void* gate, int64_t ldgate, void* dy,
                  float* part, float* part_dy, int M, int D, int T, void* stream);
/* dst bf16 [C,R] = src bf16 [R,C]^T (utility; the training path no longer needs transposed copies) */
int reed_transpose_bf16(const void* src, void* dst, int R, int C, void* stream);
/* out[n] (+)= sum_r part[r, n], f32 [R, N], fixed order; ws (optional, cdiv(R,64)*N floats) enables the two-stage
 * path for tall inputs */
int reed_rowsum_f32(const float* part, int R, float* ws, float* out, int N, int accumulate, void* stream);

/* reduce per-chunk partials to bf16 modulation grads:
 *   dmod[b, col0 + j*D + d] = bf16( sum_{c<T/16} part_j[(b*T/16 + c)*stride_j + d] ) for the listed parts */
int reed_reduce_mod_parts(const float* const* parts, const int64_t* strides, const int64_t* offs,
                          int nparts, void* dmod, int64_t lddmod, int B, int D, int chunks,
                          void* stream);

/* ---------------------------------------------------------------------------------------------
 * Attention (timm Attention under sit.py:114-118; softmax(q k^T / sqrt(hd)) v), head_dim 64 or 72 (forward only: also 80).
 * qkv bf16 [B, T, 3, H, hd] as produced by the qkv Linear; o bf16 [B, T, H*hd]; lse f32 [B,H,T].
 * ------------------------------------------------------------------------------------------- */
int reed_attention_fwd(const void* qkv, void* o, float* lse, int B, int T, int H, int hd,
                       void* stream);
/* Backward without a workspace: T <= 256 (the library allocates nothing; longer sequences take the workspace form below). */
int reed_attention_bwd(const void* qkv, const void* o, const void* d_o, const float* lse,
                       void* dqkv, int B, int T, int H, int hd, void* stream);
/* The same backward with a caller-owned workspace of reed_attention_bwd_ws_floats(B, T, H) floats (delta = rowsum(dO * O) is
 * formed there by a row kernel, which lets the main kernel run persistently with the next (batch, head) item's operands in
 * flight under the current one: csrc/attention.hip); ws == NULL falls back to reed_attention_bwd.  Replaces the autograd of
 * F.scaled_dot_product_attention inside timm Attention (image/models/sit.py:114-118).
 * T <= 256, or 256 < T <= 4096 with T % 16 == 0 (512^2 training: T = 1024), anything else is refused.  The workspace is B*T*H
 * floats for T <= 256; for T > 256 it is B*T*H*(1 + ceil(T/256)*72): delta, then one fp32 partial dQ per 256-key tile, sized for
 * head_dim 72 because the size function has no head_dim. */
int64_t reed_attention_bwd_ws_floats(int B, int T, int H);
int reed_attention_bwd_ws(const void* qkv, const void* o, const void* d_o, const float* lse, void* dqkv, float* ws,
                          int B, int T, int H, int hd, void* stream);
/* The same with delta taken from dpart f32 [H, S, B*T] (S = 1 for hd 64, 2 for hd 72): the per-row, per-head partial dot
 * products dO . O that reed_gemm's epilogue 13 leaves when it PRODUCES dO (the input gradient of the attention output
 * projection, layout NN, R = O, C2 = dpart, rows_per_gate = hd) — the 302 MB row pass over dO and O (b = 256) becomes a
 * 12 MB one, and O is not read by the backward at all.  16-bit builds; the fp32 build returns 1002. */
int reed_attention_bwd_dp(const void* qkv, const void* d_o, const float* lse, const float* dpart, void* dqkv, float* ws,
                          int B, int T, int H, int hd, void* stream);

/* qk_norm (timm Attention(qk_norm=True); reference flag --qk-norm, sit.py:114-116): LayerNorm over head_dim (eps, affine
 * f32 [hd]) on the q and k thirds of qkv bf16 [M,3,H,hd]; v copied through; stats f32 [M,2,H,2] = (mean, rstd).
 * backward: dpre = LNbwd(dn*w) (v copied); part f32 [nblocks,2(q,k),2(dw,db),hd] per-block partial parameter grads
 * (reed_qk_norm_bwd_part_floats floats), reduce with reed_rowsum_f32. */
int reed_qk_norm_fwd(const void* qkv, const float* qw, const float* qb, const float* kw, const float* kb,
                     void* out, float* stats, int M, int H, int hd, float eps, void* stream);
int64_t reed_qk_norm_bwd_part_floats(int M, int H, int hd);
int reed_qk_norm_bwd(const void* dn, const void* qkv, const float* stats, const float* qw, const float* kw,
                     void* dpre, float* part, int M, int H, int hd, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Embedders and the final layer
 * ------------------------------------------------------------------------------------------- */
/* PatchEmbed (timm, sit.py:198-200,279): tokens f32 [B,T,D] = bf16(conv_p(x bf16, W bf16)+b) + pos_embed f32 */
int reed_patch_embed_fwd(const float* x, const void* w, const void* bias, const float* pos,
                         float* tokens, int B, int C, int HW, int P, int D, void* stream);
/* PatchEmbed, input gradient (what autograd gives the reference through F.conv2d): for token bt = (b, ph, pw) and
 * k = (c, pi, pj)   dx f32 [B,C,HW,HW] at [b, c, ph*P+pi, pw*P+pj] = sum_d r(dtok[bt, d]) * w[d, k].
 * dtok is the f32 token-stream gradient [B*T, D], rounded to the operand type on load (r; the identity in the fp32 build) exactly
 * as reed_smallk_wgrad reads it with wide_is_f32 = 1; w is the stored operand-type weight [D, C*P*P].  fp32 accumulation in a
 * fixed order (two runs: the same bits).  The stride is the patch size, so every element of dx is written exactly once: no
 * atomics, no zero fill, nothing past the end.  C*P*P = 16 with D % 4 == 0, D <= 1280 and 16-byte aligned dtok / w streams
 * dtok once at 16 bytes per lane; anything else reed_patch_embed_fwd accepts takes a generic form.  Shapes outside that domain
 * (HW % P, C*P*P % 8, a non-positive extent) are refused without a launch. */
int reed_patch_embed_bwd_x(const float* dtok, const void* w, float* dx, int B, int C, int HW, int P, int D, void* stream);
/* patchify to bf16 rows: out bf16 [B*T, C*P*P]; order 0 = (c,pi,pj) (conv input, timm PatchEmbed),
 * order 1 = (pi,pj,c) (the unpatchify order of sit.py:256-269) */
int reed_patchify_bf16(const float* x, void* out, int B, int C, int HW, int P, int order, void* stream);
/* small-K weight gradient (patch-embed conv weight, final linear): deterministic two-stage reduction over M rows
 *   out[layout 0: d*KS+k | layout 1: k*Dw+d] (+)= sum_m wide[m,d] * small[m,k]   (wide f32 is bf16-rounded first)
 *   colsum_wide[d] (+)= sum_m wide[m,d];  colsum_small[k] (+)= sum_m small[m,k]   (either may be NULL)
 * ws: caller workspace of reed_smallk_wgrad_ws_floats(Dw, KS) floats. */
int64_t reed_smallk_wgrad_ws_floats(int Dw, int KS);
int reed_smallk_wgrad(const void* wide, int wide_is_f32, const void* small, float* ws, float* out,
                      float* colsum_wide, float* colsum_small, int M, int Dw, int KS, int layout,
                      int accumulate, void* stream);
/* TimestepEmbedder.positional_embedding (sit.py:45-64): out bf16 [B, dim] = [cos(t f) | sin(t f)] */
int reed_timestep_sinusoid(const float* t, void* out, int B, int dim, float max_period, void* stream);
/* its derivative with respect to t: dt f32 [B], dt[b] = sum_{k < dim/2} f_k * (cos(t f_k) * dsin[b, dim/2 + k] - sin(t f_k) * dsin[b, k])
 * with f_k and t f_k formed by the forward's own expressions; dsin f32 [B, dim] is the gradient with respect to the (unrounded)
 * table, the padding column of an odd dim contributes nothing.  One fixed-order reduction per sample.  B <= 0 or dim < 2 is
 * refused without a launch. */
int reed_timestep_sinusoid_bwd(const float* t, const float* dsin, float* dt, int B, int dim, float max_period, void* stream);
/* LabelEmbedder (sit.py:84-99): labels_out = drop ? num_classes : labels; c_out f32 [B,D] = t_emb bf16 + table f32[label];
 * silu_c bf16 [B,D] = bf16(silu(c)) (input of every adaLN linear, sit.py:126-129). table has table_rows rows; a label
 * outside [0, table_rows) (nn.Embedding raises, sit.py:98) is replaced by row 0 and *err_flag (device int, may be NULL)
 * is set to 1 — the caller reads it at its next synchronisation point. */
int reed_label_cond(const int64_t* labels, const uint8_t* drop, int num_classes, int table_rows, const float* table,
                    const void* t_emb, int64_t* labels_out, float* c, void* silu_c, int* err_flag, int B, int D,
                    void* stream);
/* backward of the conditioning vector: dc f32 [B,D] -> dt_emb bf16, dtable f32 [rows,D] += (deterministic scatter;
 * dsilu_c is the f32 grad w.r.t. silu(c), bf16-rounded inside).  dtable may be NULL (a frozen table): dt_emb alone, same bits. */
int reed_label_cond_bwd(const float* dsilu_c, const float* c, const int64_t* labels_eff, void* dt_emb,
                        float* dtable, int B, int D, void* stream);
/* FinalLayer + unpatchify (sit.py:140-158,256-269): out f32 [B,C,HW,HW] */
int reed_final_layer_fwd(const float* x, const void* shift, const void* scale, int64_t ldmod,
                         const void* w, const void* bias, float* out, float* mean, float* rstd,
                         int B, int T, int D, int C, int P, float eps, void* stream);
/* backward, row part: recompute h = bf16(modulate(LN(x))) -> hbuf bf16 [M,D]; dlin bf16 [M, P*P*C] = patchify(dout);
 * dh bf16 [M,D] = dlin @ W.  Follow with reed_ln_modulate_bwd(dh, ...) and reed_smallk_wgrad(hbuf, dlin).
 * B, T > 0 and T a square (dout is [B,C,HW,HW] with HW = sqrt(T) * P), as in the forward: anything else is refused
 * without a launch. */
int reed_final_layer_bwd_rows(const float* dout, const float* x, const float* mean, const float* rstd,
                              const void* shift, const void* scale, int64_t ldmod, const void* w,
                              void* hbuf, void* dlin, void* dh, int B, int T, int D, int C, int P,
                              void* stream);
/* mean over tokens for the text projector (sit.py:292,301): out bf16 [B,D] = bf16(mean_t x f32 [B,T,D]); backward: dx[b,t,:] +=
 * float(dmean[b,:]) / T.  B, T, D > 0 and non-null pointers, anything else is refused without a launch. */
int reed_token_mean_fwd(const float* x, void* out, int B, int T, int D, void* stream);
int reed_token_mean_bwd(const void* dmean, float* dx, int B, int T, int D, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SILoss arithmetic (loss.py:49-64,153-237)
 * Every entry point refuses B, per / half, T or Z <= 0 and null pointers without a launch.
 * ------------------------------------------------------------------------------------------- */
/* sample_posterior (train.py:84-91): out [B,half] = (moments[:, :half] + moments[:, half:] * eps) * scale + bias */
int reed_sample_posterior(const float* moments, const float* eps, float* out, int B, int64_t half,
                          float scale, float bias, void* stream);
/* path_type 0 linear, 1 cosine: xt = a x + s n, target = da x + ds n */
int reed_interpolant(const float* x, const float* noise, const float* t, float* xt, float* target,
                     int B, int64_t per, int path_type, void* stream);
/* loss[b] = mean((out-target)^2) */
int reed_mse_fwd(const float* out, const float* target, float* loss, int B, int64_t per, void* stream);
/* dout = gscale[b] * 2 (out-target) / per */
int reed_mse_bwd(const float* out, const float* target, const float* gscale, float* dout, int B,
                 int64_t per, void* stream);
/* cosine alignment: loss[b] = -mean_t <normalize(z), normalize(zt)>;  zt bf16 [B*T,Z] (projector out), z f32 */
int reed_cosine_fwd(const void* zt, const float* z, float* rowdot, float* loss, int B, int T, int Z,
                    void* stream); /* rowdot: caller scratch f32 [B*T] */
int reed_cosine_bwd(const void* zt, const float* z, const float* gscale, void* dzt, int B, int T,
                    int Z, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Optimiser side (train.py:94-105 update_ema, :402-409 clip + AdamW)
 * ------------------------------------------------------------------------------------------- */
/* partial[i] = sum of squares of chunk i (nblocks partials); finalize: norm_clip[0]=||g||, [1]=min(1,max_norm/(||g||+1e-6)) */
int reed_grad_sqnorm(const float* g, int64_t n, float* partial, int nblocks, void* stream);
int reed_clip_finalize(const float* partial, int nblocks, float max_norm, float* norm_clip, void* stream);
/* the same with dynamic loss scaling on the device (fp16 training; torch.amp.GradScaler as accelerate drives it,
 * image/train.py:401-409): scaler_state f32[4] = [scale, growth_tracker, found_inf, steps_taken]; the arena holds scale x the
 * gradients; norm_clip[0] = the true norm (inf / nan on overflow), [1] = clip coefficient / scale, 0 on overflow; the state is
 * updated as GradScaler.update() does (x backoff on overflow; x growth after growth_interval clean steps) */
int reed_clip_finalize_scaled(const float* partial, int nblocks, float max_norm, float* norm_clip, float* scaler_state,
                              float growth_factor, float backoff_factor, float growth_interval, void* stream);
/* fused clip * AdamW + EMA + 16-bit shadow over a flat arena; norm_clip may be NULL (no clipping); scaler_state (may be
 * NULL): an overflowed step leaves p, m, v untouched (EMA and shadow still run) and the bias corrections count the steps
 * actually taken (bc1 / bc2 are then ignored) */
int reed_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, void* shadow,
                   int64_t n_train, int64_t n_total, const float* norm_clip, const float* scaler_state, float lr,
                   float beta1, float beta2, float eps, float weight_decay, float bc1, float bc2, float ema_decay,
                   void* stream);
/* The two passes above over a SET of ranges of the arena (a partly frozen model: only the trainable parameters enter the norm and
 * are updated).  ranges: a DEVICE array of nranges int64 pairs [begin, end) in arena elements, sorted, disjoint, every bound a
 * multiple of 4 (arena segments are 8-aligned, so merged parameter ranges are), at most 1024 pairs; ranges_host: the same table in
 * HOST memory, which is what the argument checks read (unsorted, overlapping, empty, misaligned, past the end, too many: REED_ERR_ARG,
 * nothing launched) — the device copy is read by the kernel alone, so the call stays asynchronous.
 * reed_grad_sqnorm_ranges: partial[nblocks] = squared-norm partials over the union of the ranges inside g[0, n), for
 * reed_clip_finalize{,_scaled}; a fixed assignment of elements to blocks (the union numbered in arena order and dealt as
 * reed_grad_sqnorm deals [0, n)), no atomics, every block writes its partial (0 when idle).
 * reed_adamw_ema_ranges: reed_adamw_ema where elements of [0, n_train) inside a range get exactly its AdamW arithmetic and every
 * other element keeps p, m and v bit for bit (no weight decay, no moment decay); the EMA lerp and the 16-bit shadow still cover
 * [0, n_total); the same loss-scaler skip.  offset = the arena element p[0] (and g, m, v, ema, shadow [0]) stands for: a call on one
 * update chunk passes offset pointers and the whole table, or the part of it that meets the chunk. */
int reed_grad_sqnorm_ranges(const float* g, const int64_t* ranges, const int64_t* ranges_host, int nranges, int64_t n,
                            float* partial, int nblocks, void* stream);
int reed_adamw_ema_ranges(float* p, const float* g, float* m, float* v, float* ema, void* shadow,
                          int64_t n_train, int64_t n_total, const float* norm_clip, const float* scaler_state, float lr,
                          float beta1, float beta2, float eps, float weight_decay, float bc1, float bc2, float ema_decay,
                          const int64_t* ranges, const int64_t* ranges_host, int nranges, int64_t offset, void* stream);
int reed_cast_bf16(const float* src, void* dst, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * LoRA: low-rank adapters W' = W + s B A on a block linear (csrc/lora.hip; reed_amd/lora.py).  No counterpart in the
 * reference, whose nn.Linear a user wraps; here the adapters are merged into the GEMM operand copies, the hot GEMMs untouched.
 * R = 8, 16, 32 or 64.  "r" rounds to the build's operand type (the identity in the fp32 build).
 * ------------------------------------------------------------------------------------------- */
/* w' = w + scale * sum_j b[n, j] a[j, k]: fp32, j ascending (acc = fma(b, a, acc) from 0), then w' = fma(scale, acc, w); an update
 * that is exactly zero leaves w as it is (b == 0 reproduces r(w) bit for bit).  w f32 [N, K], a f32 [R, K], b f32 [N, R];
 * w_op [N, K] in the operand type receives r(w'), w32 f32 [N, K] receives w'; either may be NULL (not both), either may alias
 * nothing but itself.  One pass: 4 bytes read and 2 (+ 4) written per element of w.  K % 4 == 0. */
int reed_lora_merge(const float* w, const float* a, const float* b, float scale, void* w_op, float* w32, int N, int K, int R,
                    void* stream);
/* The adapters' gradients from the linear's (dy, x) pair: x [M, K], dy [M, N], a16 [R, K], b16 [N, R] in the operand type;
 *   u = r(scale * (x a16^T)) [M, R]     v = r(scale * (dy b16)) [M, R]       (THE SCALE IS APPLIED HERE, in fp32, before r)
 *   db f32 [N, R] (+)= dy^T u           da f32 [R, K] (+)= v^T x             (fp32 accumulation; accumulate: one add to the prior)
 * Fixed reduction order, no atomics: two runs give the same bits.  ws: caller-owned workspace of reed_lora_grads_ws_floats
 * floats (-1: shape outside the domain), 16-byte aligned; nothing outside the live elements of da / db is written.
 * 16-bit builds: N % 128 == 0, K % 128 == 0; fp32 build: N % 4 == 0, K % 4 == 0; any M >= 1.  Anything else is refused
 * without a launch. */
int64_t reed_lora_grads_ws_floats(int M, int N, int K, int R);
int reed_lora_grads(const void* x, const void* dy, const void* a16, const void* b16, float scale, float* da, float* db,
                    float* ws, int M, int N, int K, int R, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Samplers (samplers.py:46-104,107-187): fp64 state updates
 * ------------------------------------------------------------------------------------------- */
/* d = cfg ? d_u + s (d_c - d_u) : d_c  (model out f32 [2n or n]); x_next = x_cur + dt * (w0 d + w1 d_prev)
 * d_store (f64, optional) receives d for Heun's second stage. */
int reed_sampler_update(const double* x_cur, const float* model_out, const double* d_prev,
                        double* d_store, double* x_next, int64_t n_elems, int cfg, double cfg_scale,
                        double dt, double w0, double w1, void* stream);
/* SDE step (samplers.py:146-156): drift from velocity + score, Euler-Maruyama update */
int reed_sde_update(const double* x_cur, const float* model_out, const double* eps, double* x_next,
                    int64_t n_elems, int cfg, double cfg_scale, double t_cur, double dt,
                    int path_type, int last_step, void* stream);
/* model input f32 [2n or n] = f32(x f64) (duplicated when cfg) */
int reed_sampler_input(const double* x, float* out, int64_t n_elems, int dup, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gradient all-reduce over RCCL/xGMI (replaces accelerate->DDP bucketed all-reduce, train.py:293-295,401)
 * ------------------------------------------------------------------------------------------- */
int reed_comm_unique_id(void* out128);                       /* 128-byte ncclUniqueId */
int reed_comm_init(const void* id128, int rank, int world, void** comm_out);
int reed_comm_allreduce_avg(void* comm, float* buf, int64_t count, void* compute_stream); /* async on the comm stream, ordered after compute_stream */
/* the same average issued as ncclReduceScatter + ncclAllGather, in place (the direct form of SURVEY.md §5; count % world
 * tail elements through ncclAllReduce) */
int reed_comm_allreduce_avg_rsag(void* comm, float* buf, int64_t count, void* compute_stream);
int reed_comm_sync(void* comm, void* compute_stream);       /* compute_stream waits for all pending reductions */
int reed_comm_broadcast(void* comm, float* buf, int64_t count, int root, void* compute_stream);
/* all-gather of `bytes` bytes per rank (recv = world * bytes, rank-major), async on the comm stream, ordered after
 * compute_stream; reed_comm_sync_gather makes compute_stream wait for the gathers issued so far (not for reductions
 * queued behind them).  Used to exchange the K = local-batch factors of the adaLN weight gradient instead of
 * all-reducing the matrix (reed_amd/parallel.py). */
int reed_comm_allgather(void* comm, const void* send, void* recv, int64_t bytes, void* compute_stream);
int reed_comm_sync_gather(void* comm, void* compute_stream);
int reed_comm_destroy(void* comm);

/* ---------------------------------------------------------------------------------------------
 * Frozen CLIP image encoder, forward only: the producer of the alignment targets that
 * image/train.py:351-357 runs under autocast every step (image/models/clip_vit.py:208-230 UpdatedVisionTransformer:
 * conv1 14x14/14 -> [class token | patches] + positional embedding -> ln_pre -> ResidualAttentionBlocks (:173-195,
 * nn.MultiheadAttention + QuickGELU MLP) -> tokens without the class token; no ln_post, no projection).
 * The contractions go through reed_gemm (epilogues 0, 9 QuickGELU, 10 + bf16 residual) and reed_attention_fwd (hd 64,
 * T = 257); these are the row passes around them.
 * ------------------------------------------------------------------------------------------- */
/* out bf16 [B*(S/P)^2, Kp]: row (b, gy, gx), column c*P*P + py*P + px of img f32 [B,3,S,S]; columns >= 3 P^2 zero */
int reed_clip_im2col(const float* img, void* out, int B, int S, int P, int Kp, void* stream);
/* out bf16 [B,T,D]: row 0 = bf16(bf16(cls) + bf16(pos[0])), row t = bf16(patches[b,t-1] + bf16(pos[t])); T = patches+1 */
int reed_clip_tokens(const void* patches, const float* cls, const float* pos, void* out, int B, int T, int D,
                     void* stream);
/* out bf16 = bf16(LayerNorm_fp32(float(x bf16 [M,D]); eps) * w + b)   (clip_vit.py:159-165) */
int reed_ln_affine_bf16(const void* x, const float* w, const float* b, void* out, int M, int D, float eps,
                        void* stream);

/* ---------------------------------------------------------------------------------------------
 * The other frozen towers the reference can name (image/utils.py:73-82 mocov3, :133-147 mae, :149-160 jepa): plain pre-LN
 * ViTs (image/models/jepa.py:173-218 Attention / Block, :376-466 VisionTransformer; image/models/mae_vit.py:20-48 and
 * mocov3_vit.py:52-101 over timm's VisionTransformer) with an fp32 residual stream under autocast, LayerNorm(eps 1e-6,
 * affine), exact GELU (reed_gemm epilogue 11) and head_dim 64 or 80 (reed_attention_fwd).  Row passes:
 * ------------------------------------------------------------------------------------------- */
/* out (bf16 or f32, row stride ldo) = LayerNorm_fp32(x f32 [M,D]; eps) * w + b */
int reed_ln_affine_f32(const float* x, const float* w, const float* b, void* out, int out_is_f32, int M, int D,
                       int64_t ldo, float eps, void* stream);
/* out f32 [B,T,D]: rows t < nprefix = cls[t] + pos[t] (cls f32 [nprefix, D]: the class token, then DINOv2's register tokens
 * with zero pos rows), rows t >= nprefix = float(patches bf16[b, t - nprefix]) + pos[t]; T = nprefix + patches */
int reed_vit_tokens(const void* patches, const float* cls, int nprefix, const float* pos, float* out, int B, int T, int D,
                    void* stream);
/* preprocess_raw_image (image/train.py:53-74): raw u8 [B,3,R,R] -> out f32 [B,3,S,S]; order 0: /255 -> bicubic -> normalise
 * ('clip'), order 1: /255 -> normalise -> bicubic ('dinov2', 'jepa'); S == R: no resampling ('mocov3', 'mae').
 * mean3 / std3 are HOST pointers to 3 floats.  Bicubic = F.interpolate(mode='bicubic', align_corners=False). */
int reed_preprocess_image(const uint8_t* raw, float* out, int B, int R, int S, const float* mean3, const float* std3,
                          int order, void* stream);
/* SwiGLU as a row pass (DINOv2 ViT-g's SwiGLUFFNFused where reed_gemm has no epilogue 17: the fp32-operand library): x12 (operand
 * type) [M, ld] = x1 | x2, the output of the w12 GEMM on the UNPACKED weight; u (operand type) [M, ldu], u[m, j] = T(T(silu(x12[m, j]))
 * * x12[m, Hd + j]) with T the library's operand type: the rounding order of epilogue 17.  Every library exports it; in the 16-bit
 * ones reed_gemm(0) + this equals reed_gemm(17) bit for bit.  Hd % 8 == 0, ld >= 2 Hd, ldu >= Hd, ld and ldu multiples of 8, 16-byte
 * aligned pointers, M > 0; anything else is refused without a launch. */
int reed_swiglu_rows(const void* x12, int64_t ld, void* u, int64_t ldu, int M, int Hd, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SD-VAE decoder: `vae.decode(latents / 0.18215).sample` of image/generate.py:87,156 and
 * image/train.py:446-447 (diffusers' AutoencoderKL, not vendored in the reference: reed_amd/vae.py restates its decoder).
 * Activations are fp32 NHWC = the token matrix [B*H*W, C]; every convolution / Linear is a reed_gemm call on it (NT, epilogue 6:
 * fp32 + bias, accumulate = the residual connection); these are the passes around the contractions (csrc/vae.hip).
 * ------------------------------------------------------------------------------------------- */
/* doubles of workspace reed_groupnorm_stats needs for x f32 [B, hw, C] */
int64_t reed_groupnorm_ws_doubles(int B, int64_t hw, int C);
/* stats f32 [B, G, 2] (optional) = (mean, rstd = 1 / sqrt(biased var + eps)) of x f32 [B, hw, C] per (image, group of C / G
 * channels), fp64 sums in a fixed order; table f32 [B, 3, C] (optional; needs gamma, beta f32 [C]) = per channel
 * (mean of its group, rstd * gamma[c], beta[c]) for reed_conv_rows.  C % 4 == 0, C <= 1024. */
int reed_groupnorm_stats(const float* x, int B, int64_t hw, int C, int G, float eps, const float* gamma, const float* beta,
                         double* ws, float* stats, float* table, void* stream);
/* The row operand of a convolution as a GEMM: out (operand type) [nrows, ldo], row r - row0 = output position r = (b, y, x) of
 * the [B, Hi << upsample, Wi << upsample] grid, columns tap * C + c = a(b, y + tap / 3 - 1, x + tap % 3 - 1, c) for taps = 9
 * (zero outside the grid: padding 1) or a(b, y, x, c) for taps = 1, columns [taps * C, kcols) zero; a = x f32 [B, Hi, Wi, C]
 * read through nearest x2 upsampling when `upsample`, GroupNorm-ed as fma(x - mean, rstd * gamma, beta) with reed_groupnorm_stats'
 * table when table != NULL, SiLU-ed when `silu`.  taps = 1 is the activation pass in front of reed_conv3x3 and of the
 * attention's Linear layers.  C, kcols, ldo multiples of 4; fewer than 2^31 output positions. */
int reed_conv_rows(const float* x, const float* table, int B, int Hi, int Wi, int C, int silu, int upsample, int taps,
                   int64_t row0, int64_t nrows, int kcols, void* out, int64_t ldo, void* stream);
/* 3x3 convolution, padding 1, as an implicit GEMM (no im2col matrix: the kernel's row operand is gathered from the activation,
 * zero outside the image; 16-bit builds: csrc/conv.hip on v_mfma_f32_16x16x32, LDS-DMA gather; fp32 build: csrc/gemm_f32.hip's
 * kernel with the window gather in its staging loads): out f32 [B*Ho*Wo, ldc] (+)= conv(a) + bias, a (operand type) NHWC
 * [B, Hi, Wi, C] read through nearest x2 upsampling when `upsample` (Ho = Hi << upsample), w (operand type) [N, 9 C] in
 * (ky, kx, ci) order, bias f32 [N] or NULL; accumulate != 0 adds onto what `out` holds (the residual connection, in place).
 * 16-bit builds: C % 64 == 0, N % 128 == 0, B*Hi*Wi*C*2 bytes < 2 GiB; fp32 build: C % 4 == 0, N % 4 == 0. */
int reed_conv3x3(const void* a, const void* w, const float* bias, float* out, int64_t ldc, int B, int Hi, int Wi, int C, int N,
                 int upsample, int accumulate, void* stream);
/* p (operand type) [rows, ldp] = softmax over the first `cols` columns of scale * s f32 [rows, lds] */
int reed_softmax_rows(const float* s, int64_t lds, void* p, int64_t ldp, int rows, int cols, float scale, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SD-VAE encoder (`python -m reed_amd.dataset encode`; the reference's image/preprocessing/dataset_tools.py encode through
 * diffusers' AutoencoderKL.encode: reed_amd/vae.py restates it).  The same ResNet / attention passes as the decoder plus:
 * ------------------------------------------------------------------------------------------- */
/* 3x3 convolution at stride 2 with zero padding of one row at the bottom and one column at the right only (diffusers'
 * Downsample2D(padding=0): F.pad(x, (0, 1, 0, 1)), then the convolution): out f32 [B * (Hi / 2) * (Wi / 2), ldc] (+)= conv(a) + bias,
 * tap (ky, kx) of output (y, x) reads a(b, 2y + ky, 2x + kx), zero at or beyond Hi / Wi (odd sizes included).  Arguments as
 * reed_conv3x3; Hi, Wi >= 2. */
int reed_conv3x3_down(const void* a, const void* w, const float* bias, float* out, int64_t ldc, int B, int Hi, int Wi, int C, int N,
                      int accumulate, void* stream);
/* conv_in's row operand from the dataset's pixels: raw u8 [B, 3, H, W] -> out (operand type) [nrows, ldo], row r - row0 = position
 * r = (b, y, x) of [B, H, W], column tap * 3 + c = raw(b, c, y + tap / 3 - 1, x + tap % 3 - 1) / 127.5 - 1, 0 outside the image
 * (padding in the normalised domain), columns [27, kcols) zero.  kcols >= 28, kcols and ldo multiples of 4. */
int reed_vae_image_rows(const uint8_t* raw, int B, int H, int W, int64_t row0, int64_t nrows, int kcols, void* out, int64_t ldo,
                        void* stream);
/* The encoder's tail after conv_out: y f32 [B*h*w, ldc] (first 8 columns) -> z = quant_conv(y) (qw f32 [8, 8] as [out, in], qb f32
 * [8], fp32), mean = z[0:4], std = exp(clamp(z[4:8], -30, 20) / 2); out f32 [B, 8, h, w] = cat[mean, std] (NCHW). */
int reed_vae_moments(const float* y, int64_t ldc, int B, int h, int w, const float* qw, const float* qb, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * `python -m reed_amd.dataset convert`: Pillow's 8-bit resampler (ImagingResample behind Image.resize on uint8), the crop / resize
 * of the reference's image/preprocessing/dataset_tools.py convert (make_transform), bit for bit (csrc/resample.hip).  A resize is
 * a horizontal pass, then a vertical one, each u8 -> u8: out = clip_0_255((2^21 + sum_t in[first + t] * k[t]) >> 22) in int32.  The
 * host planner (reed_amd/resample.py) builds the int32 coefficients k as Pillow does and trims each pass to the window that later
 * passes read.
 * ------------------------------------------------------------------------------------------- */
/* One pass ("level") for a ragged batch: item j is one pass of one image, independent of the others.  Images are interleaved RGB
 * (byte 3 x + c of a row); image offsets and row pitches are multiples of 16 bytes.  Nothing is allocated and the host is never
 * waited for.
 *   items        n_items x 16 int32 words (16-byte aligned):
 *                [0:2]  int64 byte offset of the source image in `src`      [2:4]  int64 byte offset of the destination
 *                [4] source row pitch  [5] destination row pitch (bytes)      [6] source samples along the filtered axis
 *                [7] out0, [8] nout: the outputs [out0, out0 + nout) along the filtered axis are computed
 *                [9] oth0, [10] noth: over [oth0, oth0 + noth) of the other axis (columns in pixels for a vertical pass, rows
 *                     for a horizontal one); source and destination share the coordinates of that axis
 *                [11] first int32 of the item's coefficients in `coefs`    [12] first (first, taps) pair of the item in `bounds`
 *                [13] ksize: coefficients per output; output out0 + i uses bounds[[12] + i] = (first source sample, taps <= ksize)
 *                     and coefs[[11] + i * ksize + t], t < taps; first + t is clamped into [0, [6])
 *                [14] kind: 0 horizontal, 1 vertical (both into `dst`, interleaved, at the output's own coordinates: row y at
 *                     [2:4] + y * [5]), 2 vertical into `out` as planar u8 [3, nout, noth]: plane c, row i, column j of the window at
 *                     [2:4] + c * [15] + i * [5] + j (noth % 4 == 0, [2:4] % 4 == 0)        [15] plane stride in bytes (kind 2)
 *   tile_prefix  int32 [n_items + 1]: tile_prefix[j + 1] - tile_prefix[j] = ceil(work items of item j / 256), work items =
 *                kind 0: noth * (((out0 + nout + 3) >> 2) - (out0 >> 2)); kind 1: nout * (((3 (oth0 + noth) + 3) >> 2) - ((3 oth0) >> 2));
 *                kind 2: nout * noth / 4.  total_tiles = tile_prefix[n_items] = the grid.
 * Written: exactly the window of each item (no pitch padding, nothing outside it).  dst may be NULL when no item has kind 0 / 1,
 * out when none has kind 2.  n_items <= 0, total_tiles <= 0, a null table or a misaligned pointer is refused without a launch. */
int reed_resample_u8(const uint8_t* src, uint8_t* dst, uint8_t* out, const void* items, const int32_t* tile_prefix, int n_items,
                     int total_tiles, const int32_t* coefs, const int32_t* bounds, void* stream);

#ifdef __cplusplus
}
#endif
#endif

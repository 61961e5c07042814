/* frhip.h -- C ABI of libfrhip.so: the MI355X (gfx950) kernels behind the face-embedding training path.
 *
 * The reference (aanna0701/face-recognition-pytorch) is pure Python over torch; it has no FFI of its own
 * (SURVEY.md section 8b).  Each entry point below replaces the device work that one reference call site hands to
 * cuDNN / cuBLAS / ATen, cited as /root/reference file:line.  INTEGRATION.md shows the ctypes stub a reference
 * maintainer would add at that call site.
 *
 * Conventions
 *   - plain pointers to DEVICE memory owned by the caller (PyTorch caching allocator), sizes as int / size_t;
 *     no torch types; the library allocates nothing.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*); no hidden synchronisation.
 *   - returns 0 on success, a negative FRHIP_E* code otherwise; frhip_last_error() gives the message
 *     (thread-local).  Nothing throws across the boundary.
 *   - dtype: 0 = bf16 storage + bf16 MFMA (fp32 accumulate), 1 = fp32 storage + exact-fp32 MFMA (validation mode).
 *   - activations are NHWC ("channels last"); conv weights are [K][R][S][C] which is the physical layout of a
 *     torch channels_last [K,C,R,S] tensor.
 */
#ifndef FRHIP_H
#define FRHIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef FRHIP_STREAM_T
#define FRHIP_STREAM_T
#ifdef __HIP_PLATFORM_AMD__
#include <hip/hip_runtime_api.h>
typedef hipStream_t frhip_stream_t;
#else
typedef void* frhip_stream_t;
#endif
#endif

#define FRHIP_OK 0
#define FRHIP_EINVAL (-1)
#define FRHIP_ELAUNCH (-2)
#define FRHIP_DT_BF16 0
#define FRHIP_DT_F32 1

/* Threading contract.  Every compute entry point is asynchronous on the stream it is given, keeps no state between calls and may
 * be called concurrently from several host threads on different streams (frhip_last_error() is per thread).
 * The frhip_set_* functions are TEST / TUNING HOOKS, not part of that contract: they flip process-global kernel-selection
 * switches (which tile, which kernel variant -- never the arithmetic contract beyond what each hook documents), are not
 * synchronised, and must only be called while no other thread is inside the library.  The product path (nets/, model/,
 * bench.py) never changes them (one read-only query, frhip_set_winattn_mfma(-1)); the defaults are the measured-best settings, and the
 * library reads no environment variables. */
const char* frhip_last_error(void);
int frhip_abi_version(void);
/* stream-concurrency probe: one wave that occupies `stream`'s hardware queue for `ticks` of the 100-MHz wall clock (<= 1e8).
 * nets/_backbone.py times two of them on two streams to find a side stream that does not share the main stream's hardware queue. */
int frhip_spin(long long ticks, frhip_stream_t stream);

/* ---- convolution = MFMA implicit GEMM.  nn.Conv2d(bias=False): nets/resnet.py:23-46, used at :89-103, :232 ---- */
/* y[n,ho,wo,k] = conv(x[n,h,w,c], w[k,r,s,c]); stats_partial (may be NULL) receives per-row-tile
 * {sum, sum of squares} per output channel: [frhip_conv_stat_rows(...)][2][k] -- the BN batch statistics
 * (nets/resnet.py:90-91) come out of the conv epilogue instead of a second pass. */
int frhip_nt_block_m(int k);
/* number of partial rows frhip_conv_fwd writes into stats_partial for this convolution (m = n*ho*wo output pixels) */
int frhip_conv_stat_rows(int dtype, int m, int k, int h, int w, int c, int r, int s, int stride, int pad);
/* test hook: 1 (default) = 3x3 / stride-1 bf16 weight gradients on the nine-tap kernel, 0 = on the per-tap gather kernel;
 * < 0 queries.  Returns the old value */
int frhip_set_wgrad_taps9(int enabled);
/* test hook: 1 (default) = a nine-tap weight gradient takes the lane-mask table of its map geometry when one can be had (at most 8
 * geometries per process, period H W / gcd(H W, 64) <= 64, not inside a stream capture), 0 = it never asks and runs the twin that
 * tracks the padding predicates per lane; < 0 queries.  Same sums either way.  Returns the old value */
int frhip_set_wgrad_mask_table(int enabled);
/* test hook: period (in K steps) of the lane-mask table cached for h x w maps on the current device, 0 if none is cached or no device
 * is present.  Read-only: allocates nothing, launches nothing */
int frhip_wgrad_mask_table_period(int h, int w);
/* test hook: 0 disables the LDS-halo 3x3/s1 kernel (generic NT kernel is used instead), 1 automatic tile choice,
 * 2 forces the 4-wave 256x64 tile (two workgroups per CU), 3 the 8-wave 256x128 tile.  Returns the old value */
int frhip_set_conv_halo(int enabled);
/* test / tuning hook: which 3x3/s1 launches of the W <= 28 layers (bf16, automatic mode) may use the 64 x 128-per-wave halo tile:
 * bit 0 forward, bit 1 data-gradient (default 2); < 0 queries.  Returns the old value */
int frhip_set_halo_wide_dirs(int dirs);
/* test hook: 1 (default) = launches whose tiles are all whole and whose layout is dense (bf16) run the LEAN kernel instantiations
 * (32-bit buffer-offset store epilogue, BatchNorm sums on the matrix pipe); 0 = always the general store epilogue; < 0 queries.
 * Outputs are bit-identical either way, the per-tile partial sums agree to fp32 summation order.  Returns the old value */
int frhip_set_epi_lean(int enabled);
/* test hook for the element-wise BatchNorm passes (frhip_bn_apply, frhip_bn_bwd_apply and their _rs forms): 1 (default) = the batched
 * kernels (a thread requests the operands of four rows before it uses the first), 0 = the row-at-a-time kernels (one load in flight per
 * lane), kept as the reference the batched kernels are tested against; < 0 queries.  Outputs are bit-identical either way.
 * Returns the old value */
int frhip_set_ew_batch(int enabled);
/* test / micro-benchmark hook: force the NT tile (0 auto, 1 128x128, 2 256x64, 3 256x128, 4 256x256); returns the old value */
int frhip_set_nt_tile(int tile);
/* Inference (model/FR_PartialFC.py:205-211: encoder.eval(); nets/resnet.py:89-103 with BatchNorm in eval mode): convolution with the
 * eval-mode BatchNorm folded into its store epilogue, y = [relu](conv(x, w) * scale[k] + shift[k] + residual), scale / shift from
 * frhip_bn_eval_affine, residual (optional) shaped like y.  The convolution result is rounded to the compute dtype before the
 * affine map, as the unfused pair frhip_conv_fwd + frhip_bn_apply stores it: same values, one tensor pass less per BatchNorm. */
int frhip_conv_fwd_affine(int dtype, const void* x, const void* w, void* y, const float* scale, const float* shift, int relu,
                          const void* residual, int n, int h, int wd, int c, int k, int r, int s, int stride, int pad,
                          frhip_stream_t stream);
int frhip_conv_fwd(int dtype, const void* x, const void* w, void* y, float* stats_partial,
                   int n, int h, int wd, int c, int k, int r, int s, int stride, int pad, frhip_stream_t stream);
/* Read-only query: the launches of a forward convolution, as frhip_conv_fwd (mode 0), frhip_conv_fwd_affine (mode 1) or
 * frhip_conv_fwd_bnrelu (mode 2) would run it with these arguments under the current frhip_set_conv_halo, frhip_set_halo_wide_dirs,
 * frhip_set_nt_tile and frhip_set_epi_lean switches.  Same shape checks and errors as those entry points (mode 2 on a shape that
 * frhip_conv_bnrelu_fusable refuses: FRHIP_EINVAL); touches no device.  out[5] (host memory):
 *   [0] kernel family and [1] NT tile, as frhip_dgrad_route numbers them
 *   [2] store epilogue: 0 general, 1 lean (the folded BatchNorm of mode 1 exists in the lean epilogue only)
 *   [3] launches: 1, or 2 where frhip_conv_fwd_affine runs the convolution ([0] .. [2] describe it) and then frhip_bn_apply in place
 *   [4] rows of stats_partial = frhip_conv_stat_rows(...) */
int frhip_conv_fwd_route(int dtype, int n, int h, int wd, int c, int k, int r, int s, int stride, int pad, int mode, int out[5]);
/* dx[n,h,w,c] = conv_transpose(dy[n,ho,wo,k], w) (+ residual[n,h,w,c] if not NULL); wt = frhip_pack_wt(w) = [c][r][s][k].
 * autograd of nn.Conv2d w.r.t. input; the residual add is the gradient fan-in of `out += residual` (nets/resnet.py:101). */
int frhip_conv_dgrad(int dtype, const void* dy, const void* wt, void* dx, const void* residual,
                     int n, int h, int wd, int c, int k, int r, int s, int stride, int pad, frhip_stream_t stream);
/* frhip_conv_dgrad with the NEXT BatchNorm-backward reduction fused into its epilogue: dx is the upstream gradient of a
 * BatchNorm (nets/resnet.py:91, :98) whose saved input is y_bn [n,h,w,c]; stats_partial[frhip_dgrad_stat_rows(...)][2][c]
 * receives per-row-tile { sum d, sum d*(y_bn-mean)*invstd } with d = dx * (y_bn*mask_scale + mask_shift > 0) (mask_scale may
 * be NULL: no ReLU between the BN and this gradient) -- what frhip_bn_bwd_reduce would compute in a second pass over dx
 * and y_bn; feed it to frhip_bn_bwd_finalize. */
int frhip_dgrad_stat_rows(int dtype, int n, int h, int wd, int c, int k, int r, int s, int stride, int pad);
/* Read-only query: the launches of a data-gradient, as frhip_conv_dgrad / _fused / _fused_rs / _bnred would run it with these arguments
 * under the current frhip_set_conv_halo, frhip_set_halo_wide_dirs, frhip_set_nt_tile and frhip_set_epi_lean switches.  residual_stride: 0 no
 * residual, 1 dense, 2 compact; bnred != 0: with BatchNorm-backward partials (y_bn given).  Same shape checks and errors as those entry
 * points; touches no device.  out[5] (host memory):
 *   [0] kernel family: 0 the generic gather kernel, 1 / 2 / 3 the halo tiles <4,1,4,1> / <8,1,2,2> / <4,2,4,2> (waves m, waves n, 16-pixel
 *       blocks per wave, window buffers), 4 the 64 x 128-per-wave halo tile
 *   [1] NT tile of the generic kernel as frhip_set_nt_tile numbers them (1 .. 4), 0 for a halo family
 *   [2] store epilogue: 0 general, 1 lean, 2 lean in two 64-row halves (the 256 x 256 tile with BatchNorm-backward partials)
 *   [3] launches: 1, or the non-empty parity classes of a 3x3 / stride-2 / pad-1 gradient (1 .. 4); [1] and [2] describe the first and are
 *       -1 where a later class differs from it
 *   [4] rows of stats_partial = frhip_dgrad_stat_rows(...) */
int frhip_dgrad_route(int dtype, int n, int h, int wd, int c, int k, int r, int s, int stride, int pad, int residual_stride, int bnred,
                      int out[5]);
int frhip_conv_dgrad_bnred(int dtype, const void* dy, const void* wt, void* dx, const void* residual,
                           const void* y_bn, const float* mean, const float* invstd, const float* mask_scale,
                           const float* mask_shift, float* stats_partial, int n, int h, int wd, int c, int k,
                           int r, int s, int stride, int pad, frhip_stream_t stream);
/* the general form: residual_stride 1 = dense residual [n,h,w,c]; 2 = residual is the COMPACT gradient of a stride-2 1x1
 * shortcut, [n,(h+1)/2,(w+1)/2,c], added on the even pixels only (the downsample branch of nets/resnet.py:96-101: its
 * zero-stuffed full-size gradient is never built).  y_bn == NULL: no BatchNorm reduction (stats_partial ignored). */
int frhip_conv_dgrad_fused(int dtype, const void* dy, const void* wt, void* dx, const void* residual, int residual_stride,
                           const void* y_bn, const float* mean, const float* invstd, const float* mask_scale,
                           const float* mask_shift, float* stats_partial, int n, int h, int wd, int c, int k,
                           int r, int s, int stride, int pad, frhip_stream_t stream);
/* frhip_conv_dgrad_fused for a BatchNorm under stochastic depth (nets/AlterNet_SwinV2_FAN.py:407-450: x + drop_path(norm(f(x))), the
 * BatchNorm's incoming gradient is dx * rowscale[sample]): rowscale[g] (fp32: 0 for a dropped sample, keep_scale = 1 / keep-probability for
 * a kept one) covers the rows_per consecutive rows of sample g; the partial sums are those frhip_bn_bwd_reduce_rs would produce from the
 * stored dx, dx itself is stored unscaled.  Replaces that separate pass over (dx, y_bn) in the attention blocks' backward. */
int frhip_conv_dgrad_fused_rs(int dtype, const void* dy, const void* wt, void* dx, const void* residual, int residual_stride,
                              const void* y_bn, const float* mean, const float* invstd, const float* mask_scale,
                              const float* mask_shift, const float* rowscale, int rows_per, float keep_scale,
                              float* stats_partial, int n, int h, int wd, int c, int k, int r, int s, int stride, int pad,
                              frhip_stream_t stream);
/* dw[k,r,s,c] (fp32, caller-zeroed) += sum over output pixels dy * x.  autograd of nn.Conv2d w.r.t. weight.
 * splits <= 0: library picks the split-K factor.  workspace (may be NULL): caller-owned scratch used by THIS call only
 * (one per stream); when splits * sizeof(dw) fits, each K split stores a private slab with plain stores and one reduce
 * pass adds them (deterministic, no same-address atomic contention); otherwise fp32 atomics are used. */
int frhip_conv_wgrad(int dtype, const void* dy, const void* x, float* dw, int n, int h, int w, int c,
                     int k, int r, int s, int stride, int pad, int splits, float* workspace, size_t workspace_bytes,
                     frhip_stream_t stream);
/* Chained weight gradients of 3x3 / stride-1 bf16 convolutions on 14 x 14 maps (the rows kernel): launch i adds the K-split slabs of
 * launch i - 1 to THAT launch's dw in its own prologue, so no reduce launch sits between two weight gradients of a stream (inside the
 * training step the separate reduce -- 8 us alone -- took 50 - 65 us: it got onto the CUs only as the other stream's workgroups retired).
 * frhip_conv_wgrad_chain_ok: 1 when the shape is served.  frhip_conv_wgrad_chain writes this launch's slabs to `slabs` (>= *splits_out *
 * k*9*c floats; must differ from prev_slabs), stores the split count in *splits_out (host memory) and does NOT touch this launch's dw:
 * pass (dw, slabs, k, c, *splits_out) as the prev_* arguments of the next launch on the same stream, or to
 * frhip_conv_wgrad_chain_finish, which adds them with the ordinary reduce kernels.  prev_splits = 0: nothing to add.
 * Same sums in the same order as frhip_conv_wgrad on these shapes (bit-identical dw). */
int frhip_conv_wgrad_chain_ok(int dtype, int n, int h, int w, int c, int k, int r, int s, int stride, int pad);
int frhip_conv_wgrad_chain(int dtype, const void* dy, const void* x, int n, int h, int w, int c, int k, float* slabs,
                           size_t slab_bytes, float* prev_dw, const float* prev_slabs, int prev_k, int prev_c, int prev_splits,
                           int* splits_out, frhip_stream_t stream);
int frhip_conv_wgrad_chain_finish(float* dw, float* slabs, int k, int c, int splits, frhip_stream_t stream);
/* Read-only query: the launch plan of a weight gradient, as frhip_conv_wgrad (ldp = k), frhip_gemm_tn / _overwrite (h = w = r = s = stride
 * = 1, pad = 0, n = m) and frhip_conv_wgrad_bnrelu (transform = 1) would run it with these arguments and the current
 * frhip_set_wgrad_taps9 switch.  Same argument checks and errors as those entry points; touches no device.  plan_out[8] (host memory):
 *   [0] kernel family: 0 per-tap with 128-byte rows, 1 per-tap with 256-byte rows, 2 nine-tap, 3 rows (14 x 14 maps)
 *   [1] nine-tap instantiation, 100 * operand transform + 10 * lane-mask table wanted + window stages (2, 3 or 4); 0 for other families.
 *       A launch that cannot have the table (inside a stream capture before the table exists) runs the same instantiation without it
 *   [2] K splits   [3] K steps (64 pixels; rows family: images)   [4] K steps per split
 *   [5] where the splits store: 0 one split added into dw, 1 one slab of the workspace each, 2 one split that overwrites dw
 *   [6] reduce groups: 0 no reduce launch, 1 one pass over the slabs, > 1 that many group sums first, then one pass   [7] slabs per group */
int frhip_wgrad_plan(int dtype, int n, int h, int w, int c, int kc, int ldp, int r, int s, int stride, int pad, int splits,
                     int have_workspace, size_t workspace_bytes, int overwrite, int transform, int* plan_out);
/* nn.Linear forward with its epilogue fused (nets/SwinV2.py:16-32 Mlp, :150-176 qkv / proj): out[m][n] = a[m][k] . w[n][k] +
 * bias[n] (bias may be NULL), stored in `dtype`; act_out (may be NULL) = gelu(out), exact erf form, of the stored value;
 * stats_partial (may be NULL): per-tile BatchNorm partial sums of `out`, rows = frhip_conv_stat_rows(dtype, m, n, 1,1,k,1,1,1,0) */
int frhip_linear_fwd(int dtype, const void* a, const void* w, const float* bias, void* out, void* act_out,
                     float* stats_partial, int m, int n, int k, frhip_stream_t stream);
/* data-gradient of the Linear that feeds a GELU (Mlp.fc2 backward, nets/SwinV2.py:16-32): dx[m][n] = (dy[m][k] . wt[n][k]) *
 * gelu'(pre[m][n]) with pre = the saved fc1 output; stats_partial (may be NULL, rows as frhip_linear_fwd): [.][0][n] sums to
 * the column sums of dx = the gradient of fc1.bias */
int frhip_linear_dgrad_gelu(int dtype, const void* dy, const void* wt, const void* pre, void* dx, float* stats_partial,
                            int m, int n, int k, frhip_stream_t stream);
/* out[m][n] = sum_k a[m][k]*b[n][k].  atomic_f32 = 0: out has `dtype`, overwritten (splits ignored);
 * atomic_f32 = 1: out is fp32, caller-zeroed, K is split `splits` ways and added atomically.  nn.Linear: nets/resnet.py:244 */
int frhip_gemm_nt(int dtype, const void* a, const void* b, void* out, int m, int n, int k, int splits,
                  int atomic_f32, frhip_stream_t stream);
/* the same product with a deterministic K split (the fc of nets/resnet.py:244 has M = N = 512, K = 25 088): every split
 * stores a private fp32 slab into the caller's workspace, one pass adds them in split order and adds bias[n] (or NULL) */
int frhip_gemm_nt_splitk(int dtype, const void* a, const void* b, const float* bias, float* out, int m, int n, int k,
                         int splits, float* slabs, size_t slab_bytes, frhip_stream_t stream);
/* out[kc][c] (fp32, caller-zeroed) += sum_m p[m][0..kc) * q[m][0..c);  p has row pitch ldp elements. */
int frhip_gemm_tn(int dtype, const void* p, const void* q, float* out, int m, int kc, int ldp, int c,
                  int splits, float* workspace, size_t workspace_bytes, frhip_stream_t stream);
/* the same with out = (not +=): `out` need not be initialised; with a single K split (m <= 512 rows) the tiles are stored
 * plainly -- no zero fill and no atomic read-modify-write pass (the head's dW = dT^T E is 250 MB, nets/PartialFC.py:201) */
int frhip_gemm_tn_overwrite(int dtype, const void* p, const void* q, float* out, int m, int kc, int ldp, int c,
                            float* workspace, size_t workspace_bytes, frhip_stream_t stream);

/* ---- BatchNorm + element-wise glue.  nn.BatchNorm2d/1d: nets/resnet.py:81-86, :187, :196-199 ---- */
int frhip_colreduce_blocks(int rows, int c, int dtype);   /* number of partial rows frhip_colstats / _bn_bwd_reduce write */
int frhip_colstats(int dtype, const void* x, int rows, int c, float* partial, frhip_stream_t stream);
/* partial[nparts][2][c] -> batch mean / invstd, affine scale/shift, running-stat update (running_* may be NULL).
 * scratch: 64*2*c floats. */
int frhip_bn_finalize(const float* partial, int nparts, float* scratch, int c, float count,
                      const float* gamma, const float* beta, float* running_mean, float* running_var,
                      float momentum, float eps, float* mean, float* invstd, float* scale, float* shift,
                      frhip_stream_t stream);
int frhip_bn_eval_affine(int c, const float* gamma, const float* beta, const float* running_mean,
                         const float* running_var, float eps, float* scale, float* shift, frhip_stream_t stream);
/* stand-in BatchNorm state with which the generic BatchNorm-backward reduction over the stem's POOLED map (bn1 -> relu -> maxpool,
 * nets/resnet.py:232-235) yields the stem's reduction: mean = beta, invstd = gamma / (gamma^2 + (k beta)^2 + 1e-20), scale = 1, shift = 0 */
int frhip_bn_standin_state(int c, const float* gamma, const float* beta, float k, float* mean, float* invstd, float* scale,
                           float* shift, frhip_stream_t stream);
/* out = act(y*scale+shift [+ res | + res*res_scale+res_shift]);  BasicBlock tail: nets/resnet.py:92, :96-101 */
int frhip_bn_apply(int dtype, const void* y, const float* scale, const float* shift, const void* res,
                   const float* res_scale, const float* res_shift, int relu, void* out, int rows, int c,
                   frhip_stream_t stream);
/* backward of BN (optionally preceded by the ReLU mask recomputed from y*mask_scale+mask_shift > 0) */
int frhip_bn_bwd_reduce(int dtype, const void* dout, const void* y, const float* mean, const float* invstd,
                        const float* mask_scale, const float* mask_shift, int rows, int c, float* partial,
                        frhip_stream_t stream);
int frhip_bn_bwd_finalize(const float* partial, int nparts, float* scratch, int c, float count,
                          const float* gamma, const float* mean, const float* invstd, float* dgamma,
                          float* dbeta, float* ca, float* cb, float* cc, frhip_stream_t stream);
/* Eval-mode BatchNorm under differentiation (nn.BatchNorm2d in eval(): running statistics, no batch dependence).
 * frhip_bn_eval_state: frhip_bn_eval_affine's scale / shift plus mean = running_mean, invstd = rsqrt(running_var + eps), the state the
 * backward reductions (frhip_bn_bwd_reduce, the fused data-gradient epilogues, the stem's) form xhat from.
 * frhip_bn_bwd_finalize_eval: frhip_bn_bwd_finalize for such a state -- the same dgamma += sum d*xhat, dbeta += sum d, with
 * ca = gamma*invstd, cb = cc = 0 (dy = gamma*invstd*d).  Replaces the reference's autograd of F.batch_norm(training=False).
 * In both finalizes dgamma / dbeta may be NULL: only (ca, cb, cc) are written (backward for the input gradient alone). */
int frhip_bn_eval_state(int c, const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                        float* mean, float* invstd, float* scale, float* shift, frhip_stream_t stream);
int frhip_bn_bwd_finalize_eval(const float* partial, int nparts, float* scratch, int c, float count,
                               const float* gamma, const float* mean, const float* invstd, float* dgamma,
                               float* dbeta, float* ca, float* cb, float* cc, frhip_stream_t stream);
int frhip_bn_bwd_apply(int dtype, const void* dout, const void* y, const float* ca, const float* cb,
                       const float* cc, const float* mask_scale, const float* mask_shift, void* dy,
                       int rows, int c, frhip_stream_t stream);
/* stochastic depth around a normalised branch (timm DropPath as used by nets/AlterNet_SwinV2_FAN.py:407-450: x + drop_path(norm(f(x)))):
 * rowscale[g] (0 or 1/keep, fp32) multiplies the rows_per consecutive rows of sample g -- out = res + rowscale * (y*scale+shift) in the
 * forward pass, d = dout * rowscale in the BatchNorm-backward reduction and apply.  One pass each instead of separate full-tensor
 * multiply / add launches. */
int frhip_bn_apply_rs(int dtype, const void* y, const float* scale, const float* shift, const void* res, const float* rowscale,
                      int rows_per, void* out, int rows, int c, frhip_stream_t stream);
int frhip_bn_bwd_reduce_rs(int dtype, const void* dout, const void* y, const float* mean, const float* invstd, const float* rowscale,
                           int rows_per, int rows, int c, float* partial, frhip_stream_t stream);
int frhip_bn_bwd_apply_rs(int dtype, const void* dout, const void* y, const float* ca, const float* cb, const float* cc,
                          const float* rowscale, int rows_per, void* dy, int rows, int c, frhip_stream_t stream);
/* out_accum[c] += sum over partial rows of partial[p][which][c]  (fc bias gradient = column sum) */
int frhip_sum_partials(const float* partial, int nparts, int c, int which, float* out_accum, frhip_stream_t stream);
int frhip_add_bias(float* x, const float* bias, int rows, int c, frhip_stream_t stream);
int frhip_cast_from_f32(int dtype, const float* src, void* dst, size_t n, frhip_stream_t stream);
int frhip_cast_to_f32(int dtype, const void* src, float* dst, size_t n, frhip_stream_t stream);

/* ---- stem.  conv1 + bn1 + relu + maxpool: nets/resnet.py:186-189, :232-235 ---- */
/* x NCHW fp32 [b,3,h,w] -> col [b*ho*wo][64 (bf16) | 32 (f32)], k = (r*3+s)*3+ci, zero beyond 27; stride 1
 * (nets/resnet.py:186) or 2 (nets/AlterNet_SwinV2_FAN.py:652) */
int frhip_stem_im2col(int dtype, const float* x, void* col, int b, int h, int w, int stride, frhip_stream_t stream);
int frhip_bn_relu_maxpool_fwd(int dtype, const void* y, const float* scale, const float* shift, void* out,
                              uint8_t* argmax, int b, int h, int w, int c, frhip_stream_t stream);
int frhip_maxpool_bwd(int dtype, const void* dpool, const uint8_t* argmax, void* da, int b, int h, int w,
                      int c, frhip_stream_t stream);

/* ---- operand packs ---- */
int frhip_pack_wt(int dtype, const float* w, void* wt, int k, int rs, int c, frhip_stream_t stream);
/* out[cols][ld_out] = in[rows][cols]^T, ld_out >= rows, pad columns zero-filled */
int frhip_transpose2d(int dtype_in, int dtype_out, const void* in, void* out, int rows, int cols, int ld_out,
                      frhip_stream_t stream);
int frhip_pack_stem(int dtype, const float* w, void* wp, int k, int kin, int kp, frhip_stream_t stream);
int frhip_unpack_stem_grad(const float* dwp, float* dw, int k, int kin, int kp, frhip_stream_t stream);
/* fc weight columns: reference flattens NCHW (x.view(B,-1), nets/resnet.py:243); this backbone is NHWC */
int frhip_fc_permute(int dtype, const float* w, void* wp, int nout, int c, int hw, frhip_stream_t stream);
int frhip_fc_unpermute_grad(const float* dwp, float* dw, int nout, int c, int hw, frhip_stream_t stream);
/* PartialFC sampled rows: weight[index] gather (nets/PartialFC.py:120-121) / write-back (:142-143) */
/* PartialFC.sample (nets/PartialFC.py:108-121) + the shard-relative labels (:188-193) in one launch: labels[n] int64 GLOBAL class ids
 * of the gathered batch, u[num_local] the uniform draws (torch.rand on the CPU generator, :110), num_sample rows to keep.  Writes
 * *n_positive = distinct classes of this shard in the batch; if that is <= num_sample: index_out[num_sample] = the sampled rows
 * ascending (all positives + the rows with the largest draws; equal draws at the cut: lowest row first) and rel_out[n] = position of
 * the label's class in index_out, or -1 when another rank owns it.  If n_positive > num_sample (reference: `index = positive`, another
 * output length) n_positive is written, rel_out = -1 and index_out = 0 .. num_sample-1 (valid rows, to be discarded), and the caller
 * takes that branch itself.  num_local <=
 * frhip_pfc_sample_max_local(). */
int frhip_pfc_sample_max_local(void);
int frhip_pfc_sample(const int64_t* labels, int n, long long class_start, int num_local, const float* u, int num_sample,
                     int64_t* index_out, int* rel_out, int64_t* n_positive, frhip_stream_t stream);
int frhip_gather_rows(const float* src, const int64_t* index, float* dst, int n, int d, frhip_stream_t stream);
int frhip_scatter_rows(const float* src, const int64_t* index, float* dst, int n, int d, frhip_stream_t stream);

/* ---- margin-softmax head.  nets/PartialFC.py:198-207, nets/ArcFace.py:76-91, nets/PartialFC.py:441-484 ---- */
/* Head: gradient of the class centres in ONE launch (autograd of F.normalize(weight) + F.linear, nets/PartialFC.py:464-484):
 * dw[c][:] = (g[c][:] - what[c][:] * <g[c], what[c]>) * out_scale / wnorm[c] with g = dT^T ehat (dT [n][ldt] from frhip_head_bwd_dt,
 * ehat [n][512], what [classes][512] all `dtype`; wnorm, dw fp32) -- replaces frhip_gemm_tn_overwrite + frhip_l2norm_bwd, whose
 * intermediate g (250 MB at 122 000 classes) crossed HBM twice.  bf16 and d == 512 only (frhip_head_dw_ok). */
int frhip_head_dw_ok(int dtype, int n, int classes, int d);
int frhip_head_dw(int dtype, const void* dt, int ldt, const void* ehat, const void* what, const float* wnorm, float* dw,
                  int n, int classes, int d, float out_scale, frhip_stream_t stream);
/* F.normalize rows (also model/FR_PartialFC.py:171) */
int frhip_l2norm_rows(int dtype, const float* x, void* xhat, float* norms, int rows, int d, float eps,
                      frhip_stream_t stream);
int frhip_l2norm_bwd(int dtype, const float* dxhat, const void* xhat, const float* norms, float* dx,
                     int rows, int d, float out_scale, frhip_stream_t stream);
/* frhip_l2norm_bwd with the gradient of the norm itself folded in (dnorm [rows] fp32; MagFace):
 * dx = ((dxhat - xhat <dxhat, xhat>) / norm + dnorm xhat) out_scale.  dnorm = 0 gives the bits of frhip_l2norm_bwd. */
int frhip_l2norm_bwd_norm(int dtype, const float* dxhat, const void* xhat, const float* norms, const float* dnorm, float* dx,
                          int rows, int d, float out_scale, frhip_stream_t stream);
int frhip_head_groups(int num_classes);     /* rows of part_max / part_sum */
/* fused normalised-GEMM -> clamp -> ArcFace margin -> x s -> per-row max & sum-exp (this shard);
 * labels: int32 shard-relative, -1 = another shard owns the class. */
int frhip_head_fwd(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes,
                   int d, float s, float m, float* part_max, float* part_sum, float* ztarget,
                   float* rowmax, float* rowsum, frhip_stream_t stream);
int frhip_head_rescale(float* rowsum, const float* local_max, const float* global_max, int n, frhip_stream_t stream);
int frhip_head_target_prob(const float* ztarget, const int* labels, const float* rowmax, const float* rowsum,
                           float* q, int n, frhip_stream_t stream);
/* the three per-row all-reduces of the distributed CE (nets/PartialFC.py:448 MAX, :453 SUM, :459 SUM) as ONE all-gather:
 * every rank packs {local max, local sum-exp, target logit | -inf} per row ([n][3] fp32), the blocks of all ranks are
 * all-gathered ([world_size][n][3]) and merged in rank order -> global max, global sum-exp, target probability q */
int frhip_head_pack_stats(const float* ztarget, const int* labels, const float* rowmax, const float* rowsum,
                          float* packed, int n, frhip_stream_t stream);
int frhip_head_merge_stats(const float* gathered, int world_size, int n, float* rowmax, float* rowsum, float* q,
                           frhip_stream_t stream);
int frhip_head_loss(const float* q, int n, float* loss, frhip_stream_t stream);
/* dT[n][ldt] = d loss / d cos (after clamp/margin/scale chain rule); gscale = 1 / N_global, times the device
 * scalar *upstream when it is not NULL (the reference syncs the host here: loss_gradient.item(), nets/PartialFC.py:484).
 * dtt (may be NULL): the same matrix class-major, dtt[classes][ldtt] (ldtt >= n, a multiple of the 16-byte vector; columns >= n zero),
 * which the embedding-gradient GEMM (contraction over classes) reads -- written from the same tiles, no transpose pass */
int frhip_head_bwd_dt(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes,
                      int d, float s, float m, const float* rowmax, const float* rowsum, float gscale,
                      const float* upstream, void* dt, int ldt, void* dtt, int ldtt, frhip_stream_t stream);

/* Margin descriptor of the fused head and the explicit-logit margin (the three modules of the reference's nets/ArcFace.py):
 *   kind FRHIP_MARGIN_ARCFACE, easy 0: ArcFace(s, m) / CombinedMarginLoss(s, 1, m, 0) -- target t -> cos(theta + m) above cos(pi - m),
 *                                      else t - m sin(pi - m) (nets/ArcFace.py:76-91, :41-51)
 *   kind FRHIP_MARGIN_ARCFACE, easy 1: the easy_margin switch -- target t -> cos(theta + m) for t > 0, else t (:45-47, :82-84)
 *   kind FRHIP_MARGIN_COSFACE:         CosFace(s, m) / CombinedMarginLoss(s, *, *, m3 = m) -- target t -> t - m (:53-57, :94-106)
 *   filter_thr > 0:                    interclass_filtering_threshold (:28-39): every element that is not its row's target and whose
 *                                      (clamped) cosine is > filter_thr becomes 0 (logit 0, gradient 0); a row whose label is -1 on this
 *                                      shard has no exempt column.  0 = off.
 * Every logit is then x s. */
#define FRHIP_MARGIN_ARCFACE 0
#define FRHIP_MARGIN_COSFACE 1
typedef struct { int kind; int easy; float s, m, filter_thr; } frhip_margin_t;
/* frhip_head_fwd / frhip_head_bwd_dt with any margin descriptor (nets/PartialFC.py:198-207 with margin_loss = any module of
 * nets/ArcFace.py).  A plain ArcFace descriptor (easy 0, filter_thr 0) runs exactly the kernels of frhip_head_fwd / _bwd_dt. */
int frhip_head_fwd_ex(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes,
                      int d, const frhip_margin_t* margin, float* part_max, float* part_sum, float* ztarget,
                      float* rowmax, float* rowsum, frhip_stream_t stream);
int frhip_head_bwd_dt_ex(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes,
                         int d, const frhip_margin_t* margin, const float* rowmax, const float* rowsum, float gscale,
                         const float* upstream, void* dt, int ldt, void* dtt, int ldtt, frhip_stream_t stream);

/* Per-row margins (not in the reference: AdaFace, Kim et al., CVPR 2022): the target element of row i gets the angular margin
 * m_ang[i] and the additive margin m_add[i] (device vectors of n floats, indexed by row of the global batch):
 *   every cosine t = clamp(raw, -1 + eps, 1 - eps) (gradient 0 where the clamp binds); non-target logit s t;
 *   target: u = acos(t) + m_ang[i], logit s (cos(clamp(u, eps, pi - eps)) - m_add[i]), d/dt = s sin(u) / sqrt(1 - t^2) while
 *   eps <= u <= pi - eps, else 0.  Rows whose label is -1 on this shard have no target. */
typedef struct { float s, eps; const float* m_ang; const float* m_add; } frhip_margin_rows_t;
/* AdaFace's margins from the embedding norms of the global batch, ONE launch, no host synchronisation (capturable):
 *   sn = clamp(norms, 0.001, 100); mean, std (unbiased, n - 1) of sn, summed in float64 in two passes;
 *   update != 0 (training): batch_mean <- t_alpha mean + (1 - t_alpha) batch_mean, batch_std likewise, written back (fp32) and used
 *   in this same call; update == 0 (eval): the buffers are only read;
 *   k = clamp(h (sn - batch_mean) / (batch_std + eps), -1, 1); m_ang = -m k; m_add = m + m k.
 * batch_mean, batch_std: device scalars (fp32).  n < 2 or a null pointer: FRHIP_EINVAL, nothing is launched. */
int frhip_adaface_margins(const float* norms, int n, double m, double h, double t_alpha, double eps, int update, float* batch_mean,
                          float* batch_std, float* m_ang, float* m_add, frhip_stream_t stream);
/* MagFace (not in the reference: Meng et al., CVPR 2021): the margin grows with the embedding's norm and a regulariser rewards large
 * norms, so the norm becomes a quality score.  With n_i the norm of row i before normalisation, over the global batch of n rows:
 *   a_i = clamp(n_i, l_a, u_a);  m_ang[i] = l_m + (u_m - l_m) (a_i - l_a) / (u_a - l_a);  m_add[i] = 0;
 *   reg = (1 / n) sum_i g(a_i),  g(a) = a / u_a^2 + 1 / a;  loss = CE + lambda_g reg, CE being the head's cross-entropy with the
 *   logits of frhip_margin_rows_t above.  Where theta + m passes pi that is the rows clip, not the official code's cos(theta) - m sin(m).
 * frhip_magface_margins: ONE launch (one workgroup), no host synchronisation (capturable).  Fills m_ang and m_add (zeros) and writes the
 * device scalar reg (fp32), summed in float64 in an order fixed by n: the same norms give the same bits on every rank.
 * n < 1, a null pointer, u_a <= l_a or l_a <= 0: FRHIP_EINVAL, nothing is launched. */
int frhip_magface_margins(const float* norms, int n, double l_a, double u_a, double l_m, double u_m, float* m_ang, float* m_add,
                          float* reg, frhip_stream_t stream);
/* The gradient of that loss through the norms, every one of the n rows of the global batch written:
 *   dnorm[i] = [l_a < n_i < u_a] (dCE/dm_ang[i] (u_m - l_m) / (u_a - l_a) + lambda_g gscale (1 / u_a^2 - 1 / n_i^2)) upstream out_scale
 *   dCE/dm_ang[i] = s sin(u_i) (1 - q_i) gscale while the clip of u_i = theta_i + m_ang[i] to [eps, pi - eps] does not bind, else 0, from
 *   what the forward pass left: cos(u_i) = z_i / s with z_i the row's target logit, sin(u_i) = sqrt(1 - cos^2) >= 0, and
 *   q_i = exp(z_i - rowmax[i]) / rowsum[i].  A row without a target keeps the regulariser term alone.
 * packed [world_size][n][3]: the blocks of frhip_head_pack_stats of all ranks (world_size 1: this rank's own); the target logit is the
 * entry above -inf among a row's third components.  rowmax, rowsum: the GLOBAL row statistics.  gscale = 1 / n.  upstream: device
 * scalar or NULL (1), as in frhip_head_bwd_dt.  out_scale: the world size across ranks, like the embedding gradient's.
 * Whether the clip bound is read off the stored logit: it did where |z_i / s| >= cosf(eps) - 2.4e-7.  The forward kernel stores
 * s cosf(eps) (or its negative) there and z / s returns it within one ulp (6e-8); the band of two ulps of 1 also takes a row whose u
 * lies within 0.22 eps inside the clip for clipped, where the dropped term is s sin(1.22 eps) (1 - q) gscale at most.
 * Bad arguments as above, and world_size < 1, s <= 0 or eps outside (0, 0.5): FRHIP_EINVAL, nothing is launched. */
int frhip_magface_norm_grad(const float* norms, const float* packed, int world_size, int n, const float* rowmax, const float* rowsum,
                            float s, float eps, double l_a, double u_a, double l_m, double u_m, double lambda_g, double gscale,
                            const float* upstream, double out_scale, float* dnorm, frhip_stream_t stream);
/* frhip_head_fwd / frhip_head_bwd_dt with per-row margins: one more instantiation of the same kernel (two floats read per row) */
int frhip_head_fwd_rows(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes,
                        int d, const frhip_margin_rows_t* margin, float* part_max, float* part_sum, float* ztarget,
                        float* rowmax, float* rowsum, frhip_stream_t stream);
int frhip_head_bwd_dt_rows(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes,
                           int d, const frhip_margin_rows_t* margin, const float* rowmax, const float* rowsum, float gscale,
                           const float* upstream, void* dt, int ldt, void* dtt, int ldtt, frhip_stream_t stream);

/* K sub-centres per class (not in the reference: sub-center ArcFace, Deng et al., ECCV 2020).  what holds subcenters x classes rows,
 * plane-major: centre k of class c is row k * classes + c, each normalised on its own.  The cosine of (row, class) is the maximum over the
 * class's centres, an exact tie going to the lowest k; clamp, margin, filtering, x s and the row statistics then see that cosine exactly
 * as the entry points above see theirs.  `classes`, labels, part_max / part_sum (frhip_head_groups(classes) rows) and the row vectors are
 * those of one plane.
 *   forward : tsub[n] (int32) = the winning centre of the row's target, -1 where the label is -1.
 *   backward: d loss / d cos goes to the winning centre alone, the other centres of that (row, class) get an exact 0.  The same operands
 *             go through the same arithmetic as in the forward kernel, so the winners are the same bit for bit.
 *             dt[m][k * ldp + c]: ldp >= classes is the planes' column pitch and a multiple of the 16-byte vector (so classes need not be),
 *             ldt >= subcenters * ldp the row pitch; columns [classes, ldp) of every plane are written as zeros.
 *             dtt (may be NULL) [subcenters * classes][ldtt], row k * classes + c.
 * frhip_head_sub_max(): the largest subcenters served.  subcenters outside 1 .. that, a plane or the whole table beyond 2 GiB, or a bad
 * pitch: FRHIP_EINVAL, nothing is launched. */
int frhip_head_sub_max(void);
int frhip_head_fwd_sub(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d,
                       int subcenters, const frhip_margin_t* margin, float* part_max, float* part_sum, float* ztarget,
                       int* tsub, float* rowmax, float* rowsum, frhip_stream_t stream);
int frhip_head_fwd_sub_rows(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d,
                            int subcenters, const frhip_margin_rows_t* margin, float* part_max, float* part_sum,
                            float* ztarget, int* tsub, float* rowmax, float* rowsum, frhip_stream_t stream);
int frhip_head_bwd_dt_sub(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d,
                          int subcenters, const frhip_margin_t* margin, const float* rowmax, const float* rowsum,
                          float gscale, const float* upstream, void* dt, int ldt, int ldp, void* dtt, int ldtt,
                          frhip_stream_t stream);
int frhip_head_bwd_dt_sub_rows(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d,
                               int subcenters, const frhip_margin_rows_t* margin, const float* rowmax, const float* rowsum,
                               float gscale, const float* upstream, void* dt, int ldt, int ldp, void* dtt, int ldtt,
                               frhip_stream_t stream);

/* ElasticFace (not in the reference: Boutros et al., CVPR-W 2022): row i's margin is a draw g_i from N(mean, std), new at every step;
 * kind 0 (FRHIP_MARGIN_ARCFACE): m_ang[i] = g_i, m_add[i] = 0; kind 1 (FRHIP_MARGIN_COSFACE): m_ang[i] = 0, m_add[i] = g_i.  The head
 * then applies the per-row rule of frhip_margin_rows_t above (its clip of the angle at pi - eps stands where the official code has none).
 * Draws: Philox4x32-10, key = (seed low 32 bits, seed high 32 bits), counter = (i, 0, step low 32, step high 32); one round is
 *   p0 = 0xD2511F53 c0, p1 = 0xCD9E8D57 c2 (64-bit products); c <- (hi(p1) ^ c1 ^ k0, lo(p1), hi(p0) ^ c3 ^ k1, lo(p0));
 *   k0 += 0x9E3779B9, k1 += 0xBB67AE85.
 * With outputs x0 .. x3, in float64: u1 = (x0 + 0.5) 2^-32, u2 = (x1 + 0.5) 2^-32, z = sqrt(-2 ln u1) cos(2 pi u2),
 * g_i = float(mean + std z); x2, x3 are unused.  A draw depends on (seed, step, i) alone -- not on n, and not on who computes it: every
 * rank derives the draws of the whole global batch without a collective.
 * step: device scalar (int64).  update != 0 (training): read, used, and step + 1 written back by the same launch (ONE workgroup, no host
 * synchronisation, capturable); update == 0 (eval): every g_i = float(mean) and step is only read.
 * frhip_elastic_draws writes the bare draws g[n] (for frhip_elastic_assign).
 * n < 1, a null pointer, std < 0 or a kind outside {0, 1}: FRHIP_EINVAL, nothing is launched. */
int frhip_elastic_margins(int n, int kind, double mean, double std, long long seed, long long* step, int update, float* m_ang,
                          float* m_add, frhip_stream_t stream);
int frhip_elastic_draws(int n, double mean, double std, long long seed, long long* step, int update, float* g, frhip_stream_t stream);
/* The target cosine of every row on the shard that owns it (the key ElasticFace+ ranks by): tcos[i] = max over the class's `subcenters`
 * centres (plane-major, as in frhip_head_fwd_sub) of the fp32 dot of ehat[i] with what[k * classes + labels[i]]; exactly -2.0f where
 * labels[i] is -1.  One wavefront per row, 16-byte loads, the sum in an order fixed by d; no atomics.  dtype, d: those of frhip_head_fwd.
 * Bad shape / dtype, subcenters outside 1 .. frhip_head_sub_max() or a null pointer: FRHIP_EINVAL, nothing is launched. */
int frhip_head_target_cos(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d, int subcenters,
                          float* tcos, frhip_stream_t stream);
/* ElasticFace+: hand the draws out by difficulty.  tcos [world_size][n]: the frhip_head_target_cos vectors of all ranks (world_size 1:
 * this rank's own); c_i = max over ranks (-2 where no rank owns the row; a NaN counts as -2).  rank r_i = #{j : c_j > c_i, or c_j == c_i
 * and j < i}; with the draws sorted ascending, g_(0) <= ... <= g_(n-1) (equal draws in index order), row i gets g_(r_i): the largest
 * cosine gets the smallest margin, unowned rows rank last.  m_ang / m_add by kind as above.  Exact and deterministic (counting ranks, no
 * atomics) for 1 <= n <= 65536.  g must hold no NaN and must not overlap m_ang / m_add.
 * work: caller-owned device scratch of frhip_elastic_assign_workspace(n) bytes (0 for an n that is not served), 4-byte aligned.
 * Two launches.  Bad arguments or a workspace too small: FRHIP_EINVAL, nothing is launched. */
int frhip_elastic_assign_workspace(int n);
int frhip_elastic_assign(const float* tcos, int world_size, int n, const float* g, int kind, float* m_ang, float* m_add, void* work,
                         size_t work_bytes, frhip_stream_t stream);

/* CurricularFace (not in the reference: Huang et al., CVPR 2020; the official implementation's rule).  The one margin that changes the
 * NON-target logits, by a test that depends on the row.  Global batch of n rows, scale s, margin m with cos_m, sin_m,
 * theta = cos(pi - m), sinmm = m sin(pi - m) rounded once from float64, momentum alpha (0.01), module state a scalar t that starts at 0:
 *   every cosine c = clamp(raw, -1, 1), gradient 0 where the clamp binds (as in the ArcFace variant);
 *   c_i = row i's target cosine: the maximum over the ranks of the frhip_head_target_cos vectors (-2 where a rank does not own the row),
 *         clamped to [-1, 1];
 *   thr_i = c_i cos_m - sqrt(1 - c_i^2) sin_m = cos(theta_y + m), with no fallback branch (the official mask uses it this way);
 *   a row that no rank owns (c_i = -2 after the maximum, or NaN) gets thr_i = +2: nothing in it is hard;
 *   training: t <- alpha mean(c_i over the owned rows) + (1 - alpha) t BEFORE t is used (no owned row: t unchanged); eval: t is only read;
 *   target column: ArcFace's rule -- c > theta: s cos(theta_y + m), slope s (cos_m + c sin_m / sqrt(1 - c^2)); else s (c - sinmm), slope s --
 *         applied to the cosine the head kernel itself computed;
 *   non-target column of row i: c > thr_i (strictly): logit s c (t + c), d/dc = s (t + 2 c); otherwise logit s c, d/dc = s;
 *   a row whose label is -1 on this shard has no exempt column: its negatives use the thr_i the owning rank produced;
 *   no gradient flows through thr_i or t;
 *   with K sub-centres the pooled cosine (maximum over the class's centres) is compared and scaled, the gradient goes to the winner alone.
 * frhip_curricular_rows: tcos [world_size][n] -> thr[n], ONE launch of one workgroup, no host synchronisation (capturable).  The mean is
 * summed in float64 in an order fixed by n (every rank gets the same bits without a collective); thr is evaluated in float64 and rounded
 * once.  t: device scalar (fp32); update != 0: read, advanced and written back by this same launch; update == 0: not touched.
 * n < 1, world_size < 1, a null pointer, m outside [0, pi) or alpha outside [0, 1]: FRHIP_EINVAL, nothing is launched. */
int frhip_curricular_rows(const float* tcos, int world_size, int n, double m, double alpha, int update, float* t, float* thr,
                          frhip_stream_t stream);
/* The head with that rule: thr [n] from frhip_curricular_rows, t the device scalar (read by the kernels at run time, so a captured
 * graph sees each step's value).  Signatures of the _rows / _sub_rows entry points.  A null descriptor or pointer in it, or m outside
 * [0, pi): FRHIP_EINVAL, nothing is launched. */
typedef struct { float s, m; const float* thr; const float* t; } frhip_margin_curr_t;
int frhip_head_fwd_curr(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes,
                        int d, const frhip_margin_curr_t* margin, float* part_max, float* part_sum, float* ztarget,
                        float* rowmax, float* rowsum, frhip_stream_t stream);
int frhip_head_bwd_dt_curr(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes,
                           int d, const frhip_margin_curr_t* margin, const float* rowmax, const float* rowsum, float gscale,
                           const float* upstream, void* dt, int ldt, void* dtt, int ldtt, frhip_stream_t stream);
int frhip_head_fwd_sub_curr(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d,
                            int subcenters, const frhip_margin_curr_t* margin, float* part_max, float* part_sum,
                            float* ztarget, int* tsub, float* rowmax, float* rowsum, frhip_stream_t stream);
int frhip_head_bwd_dt_sub_curr(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d,
                               int subcenters, const frhip_margin_curr_t* margin, const float* rowmax, const float* rowsum,
                               float gscale, const float* upstream, void* dt, int ldt, int ldp, void* dtt, int ldtt,
                               frhip_stream_t stream);

/* The sigmoid (binary cross-entropy) head (not in the reference: UniFace, Zhou et al., ICCV 2023; SphereFace2, Wen et al., ICLR 2022).
 * Every (row, class) pair is a binary problem with ONE threshold b, so no element needs its row's statistics: the recompute kernel reads
 * no row max / sum, and the ranks exchange two scalars per step instead of [n][3] triples.  With c = clamp(raw, -1, 1), gradient 0 where
 * the clamp binds (loss and bias terms still count), with K sub-centres the pooled cosine, y_i the shard-relative label (-1: no target
 * column on this shard), b = *bias read on the device by every launch (no host synchronisation, capturable):
 *   target:     a = s phi(c) - b; kind COSFACE: phi = c - m, slope 1; kind ARCFACE: ArcFace's rule, cos(theta + m) above cos(pi - m),
 *               c - m sin(pi - m) below, with its slope; term w_pos softplus(-a), d/dc = -w_pos sigmoid(-a) s slope, d/db = +w_pos sigmoid(-a);
 *   non-target: a = s (c + m_neg) - b; term w_neg softplus(a), d/dc = w_neg sigmoid(a) s, d/db = -w_neg sigmoid(a);
 *   loss = (1 / N_global) sum of the terms over all rows and all (activated) classes of all shards, dbias the same sum of the d/db;
 *   classes >= `classes` of the last tile and rows >= n contribute exactly 0 to loss, dbias and dT (a padded column's cosine is 0: unmasked
 *   it would add softplus(-b));
 *   softplus(x) = max(x, 0) + log1p(exp(-|x|)); sigmoid(a) = (a >= 0 ? 1 : e) / (1 + e), e = exp(-|a|): relative accuracy in both tails.
 * A descriptor is refused (FRHIP_EINVAL with a frhip_last_error text, nothing is launched) when it or its bias is null, kind is neither
 * FRHIP_MARGIN_ARCFACE nor _COSFACE, s is not positive and finite, m or m_neg is not finite, ARCFACE has m outside [0, pi), a weight is
 * negative or not finite, or both weights are 0. */
typedef struct { int kind; float s, m, m_neg, w_pos, w_neg; const float* bias; } frhip_margin_bce_t;
/* Forward: part_loss / part_db [frhip_head_groups(classes)][n]: the loss and bias-gradient partial sums of each 64-class column group
 * (fp32, unscaled); ztarget[i] = a of row i's target (untouched where y_i = -1); tsub as in frhip_head_fwd_sub.  A second launch folds
 * the partials into rowloss[n], rowdb[n] in float64, in group order (an order that depends on the shape alone).  Bad shape / dtype,
 * subcenters outside 1 .. frhip_head_sub_max(), a null pointer or a bad descriptor: FRHIP_EINVAL, nothing is launched. */
int frhip_head_fwd_bce(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d,
                       const frhip_margin_bce_t* margin, float* part_loss, float* part_db, float* ztarget, float* rowloss, float* rowdb,
                       frhip_stream_t stream);
int frhip_head_fwd_sub_bce(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d, int subcenters,
                           const frhip_margin_bce_t* margin, float* part_loss, float* part_db, float* ztarget, int* tsub, float* rowloss,
                           float* rowdb, frhip_stream_t stream);
/* Recompute: dT / dTt as frhip_head_bwd_dt / _sub write them, = d loss / d cos x gscale (x *upstream when not NULL).  Takes no row
 * statistics.  Bad pitches are refused as there. */
int frhip_head_bwd_dt_bce(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d,
                          const frhip_margin_bce_t* margin, float gscale, const float* upstream, void* dt, int ldt, void* dtt, int ldtt,
                          frhip_stream_t stream);
int frhip_head_bwd_dt_sub_bce(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d, int subcenters,
                              const frhip_margin_bce_t* margin, float gscale, const float* upstream, void* dt, int ldt, int ldp, void* dtt,
                              int ldtt, frhip_stream_t stream);
/* rowloss[n], rowdb[n] -> pair[2] = {sum of rowloss, sum of rowdb}: this rank's UNSCALED sums.  ONE workgroup, float64 accumulation in
 * an order fixed by n, rounded once to fp32.  n < 1 or a null pointer: FRHIP_EINVAL. */
int frhip_bce_reduce(const float* rowloss, const float* rowdb, int n, float* pair, frhip_stream_t stream);
/* gathered [world_size][2]: the pairs of all ranks (world_size 1: this rank's own) -> loss[0] = (sum_r pair_r[0]) / n_global,
 * dbias[0] = (sum_r pair_r[1]) / n_global, folded in rank order in float64 (every rank gets the same bits).  The 1 / N_global scaling
 * is applied HERE, once.  world_size < 1, n_global < 1 or a null pointer: FRHIP_EINVAL. */
int frhip_bce_merge(const float* gathered, int world_size, int n_global, float* loss, float* dbias, frhip_stream_t stream);

/* ---- bn1 -> relu -> conv2 of a BasicBlock (nets/resnet.py:91-93) WITHOUT the activated tensor: the BatchNorm-apply + ReLU
 * is folded into the operand path of the convolution (forward) and of its weight gradient, which read the saved BatchNorm
 * INPUT x and form relu(x * in_scale[c] + in_shift[c]) in LDS.  bf16, 3x3 / stride 1 / pad 1; *_fusable() tells whether a
 * shape is served (otherwise use frhip_bn_apply + the plain entry points).  Results are bit-identical to the unfused pair. ---- */
int frhip_conv_bnrelu_fusable(int dtype, int h, int wd, int c, int k, int r, int s, int stride, int pad);
/* act_out (may be NULL): [n,h,wd,c] like x -- the activated tensor relu(x * in_scale + in_shift) is written there on the way (each
 * row once, by the workgroups of output-channel column 0) for a backward pass that wants it: the forward pass then has neither
 * the BatchNorm-apply launch nor its re-read of x, and the backward pass is the unfused one */
int frhip_conv_fwd_bnrelu(int dtype, const void* x, const float* in_scale, const float* in_shift, const void* w, void* y,
                          float* stats_partial, void* act_out, int n, int h, int wd, int c, int k, int r, int s, int stride,
                          int pad, frhip_stream_t stream);
int frhip_conv_wgrad_bnrelu_fusable(int dtype, int n, int h, int w, int c, int k, int r, int s, int stride, int pad);
int frhip_conv_wgrad_bnrelu(int dtype, const void* dy, const void* x, const float* in_scale, const float* in_shift,
                            float* dw, int n, int h, int w, int c, int k, int r, int s, int stride, int pad, int splits,
                            float* workspace, size_t workspace_bytes, frhip_stream_t stream);

/* ---- fp8 weight path (BASELINE cfg 5; the reference has no fp8 arithmetic, see csrc/igemm_fp8.hip).  Forward convolutions
 * (nets/AlterNet_SwinV2_FAN.py:520-568, nets/resnet.py:23-46) and linears (:263-302) with both MFMA operands in OCP fp8
 * e4m3 on v_mfma_scale_f32_16x16x128_f8f6f4; bf16 output = fp32 accumulator x act_scale x w_scale[k] ---- */
/* w [k][rowlen] fp32 (a conv weight in its physical [K][R][S][C] order) -> w8 fp8 + scale[k] = amax(row) / 448 */
int frhip_quant_fp8_weights(const float* w, void* w8, float* scale, int k, int rowlen, frhip_stream_t stream);
/* the same for all weight tensors of a step in ONE launch (the weights change every optimizer step, model/FR_PartialFC.py:166-170):
 * row_begin = number of output rows of the tensors before this one, nrows = the total; rowlen % 4 == 0.  Table in device memory */
typedef struct { const float* w; void* w8; float* scale; int32_t k, rowlen, row_begin, pad_; } frhip_q8w;
int frhip_quant_fp8_weights_multi(const frhip_q8w* table, int ntensors, int nrows, frhip_stream_t stream);
/* debug counter of SATURATED activations in the fp8 quantisers (frhip_quant_fp8, frhip_bn_apply_q8 clamp at +-448 silently; the
 * activation scale is static): op 1 zeroes and arms it, op 0 disarms, op 2 returns the number of elements that exceeded e4m3's range
 * since it was armed (synchronises the device; capped at INT_MAX).  Process-global test hook, outside the threading contract */
int frhip_fp8_saturation(int op);
/* x8 = fp8(x * inv_scale), n % 16 == 0 */
int frhip_quant_fp8(int dtype, const void* x, void* x8, size_t n, float inv_scale, frhip_stream_t stream);
/* frhip_bn_apply that also writes the fp8 copy out8 = fp8(out * inv_q) the next fp8 GEMM reads (bf16 tensors) */
int frhip_bn_apply_q8(int dtype, const void* y, const float* scale, const float* shift, const void* res,
                      const float* res_scale, const float* res_shift, int relu, void* out, void* out8, float inv_q,
                      int rows, int c, frhip_stream_t stream);
/* y bf16 [n,ho,wo,k] = conv(x8 [n,h,w,c] fp8, w8 [k,r,s,c] fp8) * act_scale * wscale[k]; c % 128 == 0;
 * stats_partial: [frhip_fp8_stat_rows(n*ho*wo, k)][2][k] BatchNorm partial sums of the stored values, or NULL */
int frhip_conv_fwd_fp8(const void* x8, const void* w8, const float* wscale, float act_scale, void* y,
                       float* stats_partial, int n, int h, int wd, int c, int k, int r, int s, int stride, int pad,
                       frhip_stream_t stream);
int frhip_fp8_stat_rows(int m, int k);                                               /* linears / generic kernel */
int frhip_fp8_conv_stat_rows(int m, int k, int h, int w, int c, int r, int s, int stride, int pad);   /* convolutions */
int frhip_set_fp8_halo(int enabled);     /* test hook: 3x3 stride-1 fp8 convs on the LDS-halo kernel (1, default) or the generic one (0); < 0: query */
/* out bf16 [m][n] = a8 [m][k] x w8 [n][k]^T * act_scale * wscale[n] + bias[n] */
int frhip_linear_fwd_fp8(const void* a8, const void* w8, const float* wscale, float act_scale, const float* bias,
                         void* out, float* stats_partial, int m, int n, int k, frhip_stream_t stream);

/* ---- continuous position bias of the window attention (nets/SwinV2.py:88-125, :150-158; nets/AlterNet_SwinV2_FAN.py:210-283):
 * bias[h][i][j] = 16 sigmoid(cpb_mlp(coords)[index[i][j]][h]), scale[h] = exp(min(logit_scale[h], ln 100)), and the gradients of
 * cpb_mlp.0.weight / .0.bias / .2.weight / logit_scale, for ALL attention blocks of a step in one launch each way.
 * One descriptor per block (device array); every pointer is a device address, fp32 unless noted. ---- */
typedef struct frhip_cpb_block {
    const void* coords;        /* [entries][2]  relative_coords_table */
    const void* index;         /* int64 [tokens*tokens]  relative_position_index */
    const void* w0;            /* [512][2] */
    const void* b0;            /* [512] */
    const void* w2;            /* [heads][512] */
    const void* logit_scale;   /* [heads] */
    void* bias;                /* out: [heads][tokens][tokens] */
    void* scale;               /* out: [heads] */
    const void* dbias;         /* backward in: [heads][tokens][tokens] */
    const void* dscale;        /* backward in: [heads] */
    void* dw0;                 /* backward, accumulated into: same shapes as w0 / b0 / w2 / logit_scale */
    void* db0;
    void* dw2;
    void* dlogit_scale;
    int entries, tokens, heads, pad_;
} frhip_cpb_block;
int frhip_cpb_limits(int* max_entries, int* max_heads, int* hidden);
int frhip_cpb_scratch_floats(int nblocks);      /* size of the caller-owned scratch both calls need (keep it from fwd to bwd: not required) */
int frhip_cpb_fwd(const frhip_cpb_block* blocks_dev, int nblocks, float* scratch, frhip_stream_t stream);
int frhip_cpb_bwd(const frhip_cpb_block* blocks_dev, int nblocks, float* scratch, frhip_stream_t stream);

/* ---- explicit-logit margin and softmax-CE (stand-alone use of nets/ArcFace.py:76-105, nets/PartialFC.py:441-484) ---- */
/* logits[n][c] fp32 in place: target entry -> margin (kind 0 ArcFace, 1 CosFace), everything x s; tsave[n] = raw target cos.
 * labels int64 [n], -1 = no target in this shard */
int frhip_margin_fwd(float* logits, const int64_t* labels, int n, int c, float s, float m, int kind, float* tsave,
                     frhip_stream_t stream);
int frhip_margin_bwd(const float* gout, const int64_t* labels, const float* tsave, int n, int c, float s, float m,
                     int kind, float* gin, frhip_stream_t stream);
/* the same with a margin descriptor (frhip_margin_t above): CombinedMarginLoss.forward with interclass filtering
 * (nets/ArcFace.py:28-39) and the easy_margin switch (:45-47, :82-84).  filtered[n][(c + 63) / 64] (may be NULL when
 * filter_thr == 0): bit j % 64 of word j / 64 of a row is set where element j was filtered; the forward writes it, the backward
 * reads it (logits are overwritten in place, so the mask cannot be recomputed from them). */
int frhip_margin_fwd_ex(float* logits, const int64_t* labels, int n, int c, const frhip_margin_t* margin, float* tsave,
                        uint64_t* filtered, frhip_stream_t stream);
int frhip_margin_bwd_ex(const float* gout, const int64_t* labels, const float* tsave, const uint64_t* filtered, int n, int c,
                        const frhip_margin_t* margin, float* gin, frhip_stream_t stream);
/* per-row margins (frhip_margin_rows_t above; AdaFace.forward stand-alone).  NOT in place: out[n][c] = s x margin(logits), and the
 * backward reads the caller's untouched logits to see where the clamp to [-1 + eps, 1 - eps] bound (gradient 0 there). */
int frhip_margin_fwd_rows(const float* logits, const int64_t* labels, int n, int c, const frhip_margin_rows_t* margin, float* out,
                          frhip_stream_t stream);
int frhip_margin_bwd_rows(const float* gout, const float* logits, const int64_t* labels, int n, int c,
                          const frhip_margin_rows_t* margin, float* gin, frhip_stream_t stream);
/* CurricularFace (frhip_margin_curr_t above; CurricularFace.forward stand-alone) on explicit cosines, thr [n] one threshold per row.
 * NOT in place, like the _rows pair: the backward rebuilds the hard mask and the clamp from the caller's untouched logits. */
int frhip_margin_fwd_curr(const float* logits, const int64_t* labels, int n, int c, const frhip_margin_curr_t* margin, float* out,
                          frhip_stream_t stream);
int frhip_margin_bwd_curr(const float* gout, const float* logits, const int64_t* labels, int n, int c,
                          const frhip_margin_curr_t* margin, float* gin, frhip_stream_t stream);
/* The sigmoid head's rule (frhip_margin_bce_t above; UniFace.forward stand-alone) on explicit cosines [n][c], int64 labels (-1: no
 * target).  fwd: rowloss[i] / rowdb[i] = the UNSCALED sums of row i's loss and bias-gradient terms (float64 accumulation; feed
 * frhip_bce_reduce / frhip_bce_merge).  bwd: gin[i][j] = d term / d logits x gscale (x *upstream when not NULL), 0 where the clamp binds.
 * Logits stay untouched.  n < 1, c < 1, a null pointer or a bad descriptor: FRHIP_EINVAL, nothing is launched. */
int frhip_bce_fwd(const float* logits, const int64_t* labels, int n, int c, const frhip_margin_bce_t* margin, float* rowloss,
                  float* rowdb, frhip_stream_t stream);
int frhip_bce_bwd(const float* logits, const int64_t* labels, int n, int c, const frhip_margin_bce_t* margin, float gscale,
                  const float* upstream, float* gin, frhip_stream_t stream);
int frhip_rows_max(const float* x, int n, int c, float* rowmax, frhip_stream_t stream);
int frhip_rows_exp_sum(float* x, int n, int c, const float* rowmax, float* rowsum, frhip_stream_t stream);
int frhip_rows_normalize(float* x, int n, int c, const float* rowsum, const int64_t* labels, float* ptarget,
                         frhip_stream_t stream);
int frhip_ce_grad(float* p, int n, int c, const int64_t* labels, float inv_n, const float* upstream,
                  frhip_stream_t stream);

/* ---- SwinV2 window attention (ws x ws windows, ws <= 7, head dim 32).  nets/SwinV2.py:139-179 and
 * nets/AlterNet_SwinV2_FAN.py:263-302; window_partition/reverse, the cyclic roll and the SW-MSA mask
 * (nets/AlterNet_SwinV2_FAN.py:375-397, :420-440) are index arithmetic inside the kernel ---- */
/* qkv [b*h*w][3c] (pixel order), bias fp32 [heads][n][n] (n = ws*ws) = 16*sigmoid(cpb table)[index], scale fp32 [heads] =
 * exp(min(logit_scale, ln 100)); shift = 0 (W-MSA) or ws/2 (SW-MSA); out [b*h*w][c] */
int frhip_winattn_fwd(int dtype, const void* qkv, const float* bias, const float* scale, void* out, int b, int h,
                      int w, int c, int heads, int ws, int shift, frhip_stream_t stream);
/* dqkv [b*h*w][3c]; dbias [heads][n][n] and dscale [heads] are fp32, caller-zeroed; the sums over windows are added into them in a
 * fixed order (run-to-run identical): each workgroup stores its partial sums to `workspace` (need not be initialised; at least
 * heads x ~1024/heads slots of (49*49 + 97) floats -- the 160-MB split-K workspace of frhip.ops.workspace), one pass adds them */
int frhip_winattn_bwd(int dtype, const void* qkv, const void* dout, const float* bias, const float* scale,
                      void* dqkv, float* dbias, float* dscale, int b, int h, int w, int c, int heads,
                      int ws, int shift, float* workspace, size_t workspace_bytes, frhip_stream_t stream);
/* frhip_winattn_bwd that also accumulates dqkv_colsum[3c] (fp32, caller-zeroed) += column sums of the stored dqkv = the
 * gradients of q_bias / v_bias (nets/SwinV2.py:150-154).  bf16 with the MFMA kernels only; FRHIP_EINVAL otherwise */
int frhip_winattn_bwd_colsum(int dtype, const void* qkv, const void* dout, const float* bias, const float* scale,
                             void* dqkv, float* dbias, float* dscale, float* dqkv_colsum, int b, int h, int w, int c,
                             int heads, int ws, int shift, float* workspace, size_t workspace_bytes, frhip_stream_t stream);
/* frhip_winattn_bwd_colsum with the q third of the column sums added into dq_bias[c] and the v third into dv_bias[c] (fp32
 * gradient accumulators of q_bias / v_bias, nets/SwinV2.py:150-154; either may be NULL); the k third is not formed */
int frhip_winattn_bwd_qvbias(int dtype, const void* qkv, const void* dout, const float* bias, const float* scale,
                             void* dqkv, float* dbias, float* dscale, float* dq_bias, float* dv_bias, int b, int h, int w,
                             int c, int heads, int ws, int shift, float* workspace, size_t workspace_bytes, frhip_stream_t stream);
/* 1 (default): bf16 calls run the MFMA-tile kernels (bf16 GEMM operands, fp32 scores / softmax -- the reference's autocast
 * numerics); 0: the fp32-arithmetic VALU kernels for every dtype.  Negative: query.  Returns the old value */
int frhip_set_winattn_mfma(int enabled);
/* y[rows][c] += bias (in place); act_out (may be NULL) = gelu(y).  Mlp fc1 + GELU: nets/SwinV2.py:16-32 */
int frhip_bias_gelu_fwd(int dtype, void* y, const float* bias, void* act_out, int rows, int c, frhip_stream_t stream);
int frhip_gelu_bwd(int dtype, const void* da, const void* h, void* dh, size_t n, frhip_stream_t stream);

/* ---- verification metrics: utils/eval.py:68-99 pair_score.  scores[n] float64, hist_idx[n] = int(99999*score),
 * hist_genuine / hist_imposter int32[100001] (caller-zeroed) ---- */
int frhip_pair_score(const float* e1, const float* e2, const int64_t* labels, int n, int d, double* scores,
                     int* hist_idx, int* hist_genuine, int* hist_imposter, frhip_stream_t stream);
/* utils/eval.py:102-137 cross_score: all pairs j < i of ONE embedding set e [n][d] in the reference's order
 * l = i (i - 1) / 2 + j; scores / pair_labels float64 [n (n - 1) / 2] (pair label 1.0 = same identity), hist_idx int32 */
int frhip_cross_score(const float* e, const int64_t* labels, int n, int d, double* scores, double* pair_labels,
                      int* hist_idx, int* hist_genuine, int* hist_imposter, frhip_stream_t stream);
/* utils/eval.py:102-137 cross test without the pair list: the pairs (i, j < i) with i in the band [i0, i1) of e [n][d] ADD into
 * four uint64 histograms that the caller zeroes once; launches over disjoint bands that cover [0, n) accumulate the whole
 * triangle, in any order and split, to the same counts.  Same per-pair arithmetic as frhip_cross_score (float64 sum of squared
 * float32 differences in ascending k, score = 1 - sum / 4).
 *   hist_genuine / hist_imposter [100001]: the reference's bins int(99999 * score), pairs whose bin lies in [0, 100000] only --
 *     equal to frhip_cross_score's histograms.
 *   thr_genuine / thr_imposter [100002]: every pair with a non-NaN score, in slot t = the smallest t in [0, 100001] with
 *     score <= t / 1e5 (correctly rounded double quotient; <= 0 -> 0, > 1 -> 100001).  For an integer th in [0, 100000]:
 *     #{genuine: score <= th / 1e5} = sum_{t <= th} thr_genuine[t], #{imposter: score > th / 1e5} = sum_{t > th} thr_imposter[t].
 * Device memory stays O(n d) at any n.  Bad arguments (n < 0, d <= 0, a band outside [0, n]) return FRHIP_EINVAL. */
int frhip_cross_hist(const float* e, const int64_t* labels, int64_t n, int d, int64_t i0, int64_t i1, uint64_t* hist_genuine,
                     uint64_t* hist_imposter, uint64_t* thr_genuine, uint64_t* thr_imposter, frhip_stream_t stream);
/* 1:N identification (not in the reference): for every row of probe [p][d] the k best rows of the band [g0, g1) of gallery [g][d],
 * MERGED into the lists top_score [p][k] float64 / top_index [p][k] int64, which the caller initialises once to -inf / -1; calls
 * over disjoint bands that cover [0, g) leave, in any order and split, the lists of one call.  The P x G scores are never written.
 *   score : frhip_cross_score's, to the bit (float64 sum of squared float32 differences gallery - probe in ascending column,
 *           score = 1 - sum / 4).
 *   order : total -- score descending, then gallery index ascending; exact ties come out lowest index first.
 *   a pair with a NaN score is never listed; unfilled slots (fewer than k candidates) hold index -1, score -inf, at the end.
 *   exclude [p] (NULL = none): the one gallery row that probe i must not match, -1 for none (exclude[i] = i: leave-one-out).
 *   1 <= k <= 64, 1 <= d <= 2^27 (any d, not only multiples of the K chunk).  workspace: frhip_gallery_topk_workspace(p, k, &bytes) bytes, written before it is read; it holds the
 *   lists of the gallery splits of one launch, 2 MiB x k or one list per probe row if that is more.
 * p = 0 or an empty band: nothing to do.  Bad arguments (negative sizes, k out of range, a band outside [0, g], null pointers
 * with work to do, a workspace too small) return FRHIP_EINVAL. */
int frhip_gallery_topk(const float* probe, const float* gallery, const int64_t* exclude, int64_t p, int64_t g, int d, int k,
                       int64_t g0, int64_t g1, double* top_score, int64_t* top_index, void* workspace, size_t workspace_bytes,
                       frhip_stream_t stream);
int frhip_gallery_topk_workspace(int64_t p, int k, int64_t* bytes);

/* ---- recompute-style stem (stride 1): conv3x3(3->64) -> BN -> ReLU -> MaxPool(3,2,1) of nets/resnet.py:232-235 without ever
 * writing the conv output map or an im2col matrix; every pass recomputes the conv from x [b,3,h,w] fp32 NCHW and
 * wp = frhip_pack_stem(w, 64, 27, 32) ([64][32] in `dtype`).  frhip_stem_blocks(b,h,w) = partial rows / slabs the
 * grid-stride kernels write.
 *   stats      : partial[blocks][2][64] = per-workgroup { sum y, sum y^2 }            -> frhip_bn_finalize
 *   fwd        : pooled [b,hp,wp,64] `dtype`, argmax uint8 [b,hp,wp,64] (first max in row-major window order)
 *   bwd_reduce : partial[blocks][2][64] = { sum d, sum d*(y-mean)*invstd }, d = maxpool_bwd(dpool) * (y*scale+shift > 0)
 *                                                                                     -> frhip_bn_bwd_finalize
 *   bwd_wgrad  : dy = ca*d + cb*y + cc; dw[64][27] (fp32) += sum_pixels dy x im2col; slabs: blocks*64*32 floats of scratch */
int frhip_stem_blocks(int b, int h, int w);
/* test hook: 0 = gather-form backward kernels for bf16 as well (fp32 always uses them); returns the old value */
int frhip_set_stem_scatter(int enabled);
int frhip_stem_stats(int dtype, const float* x, const void* wp, int b, int h, int w, float* partial, frhip_stream_t stream);
int frhip_stem_fwd(int dtype, const float* x, const void* wp, const float* scale, const float* shift, void* pooled,
                   uint8_t* argmax, int b, int h, int w, frhip_stream_t stream);
int frhip_stem_bwd_reduce(int dtype, const float* x, const void* wp, const void* dpool, const uint8_t* argmax,
                          const float* mean, const float* invstd, const float* scale, const float* shift, int b, int h,
                          int w, float* partial, frhip_stream_t stream);
int frhip_stem_bwd_wgrad(int dtype, const float* x, const void* wp, const void* dpool, const uint8_t* argmax,
                         const float* ca, const float* cb, const float* cc, const float* scale, const float* shift, int b,
                         int h, int w, float* slabs, float* dw, frhip_stream_t stream);
/* The same weight gradient without recomputing the convolution (csrc/stem_algebra.hip): dy = ca d + cb y + cc and y = W col give
 * dW = ca D + cb (W G) + cc s with G = sum_p col col^T (27 x 27) and s = sum_p col, functions of the input batch alone, and
 * D = sum over pooled elements with pooled > 0 of dpool x col[arg-max pixel].  frhip_stem_gram fills gram[frhip_stem_gram_floats()]
 * = {G, s} from x (partial: scratch of (frhip_stem_gram_blocks(b,h,w) + 1) x 567 floats); it needs nothing else of the step, so a caller
 * can run it on a second stream during the forward pass.  frhip_stem_bwd_wgrad_gram then needs dpool, the pooled map the forward
 * pass returned (ReLU mask: pooled > 0), the arg-max bytes and (ca, cb, cc) of frhip_bn_bwd_finalize; slabs as above. */
int frhip_stem_gram_floats(void);
int frhip_stem_gram_blocks(int b, int h, int w);
int frhip_stem_gram(int dtype, const float* x, int b, int h, int w, float* partial, float* gram, frhip_stream_t stream);
int frhip_stem_bwd_wgrad_gram(int dtype, const float* x, const void* wp, const void* dpool, const void* pooled,
                              const uint8_t* argmax, const float* gram, const float* ca, const float* cb, const float* cc,
                              int b, int h, int w, float* slabs, float* dw, frhip_stream_t stream);
/* Image gradient of the stem: dx [b,3,h,w] fp32 NCHW (the layout of x), every element written once, no atomics (run-to-run identical).
 * Replaces the reference's autograd of conv1 -> bn1 -> relu -> maxpool with respect to the image (nets/resnet.py:232-235).
 * frhip_stem_dx (stride 1, recompute-style stem): dy0 = ca*d + cb*y + cc with d = dpool routed to its arg-max pixel where pooled > 0 (the
 *   ReLU mask), y = conv(x) recomputed (never stored); dx = conv^T(dy0).  dpool / pooled [b,hp,wp,64] `dtype`, argmax as
 *   frhip_stem_fwd wrote it, wp = frhip_pack_stem(w, 64, 27, 32), (ca, cb, cc) from frhip_bn_bwd_finalize(_eval).  cb = cc = NULL: the
 *   eval-mode form dy0 = ca*d (frhip_bn_bwd_finalize_eval's cb = cc = 0) -- no recompute, x may be NULL.
 * frhip_stem_dx_s2 (stride 2, im2col stem): dx = col2im(dy0 W^T) for conv3x3 / stride 2 / pad 1; dy0 [b, (h-1)/2+1, (w-1)/2+1, 64]
 *   `dtype` (the BatchNorm-backward output), wp = frhip_pack_stem(w, 64, 27, kp) ([64][kp] `dtype`). */
int frhip_stem_dx(int dtype, const float* x, const void* wp, const void* dpool, const uint8_t* argmax, const void* pooled,
                  const float* ca, const float* cb, const float* cc, int b, int h, int w, float* dx, frhip_stream_t stream);
int frhip_stem_dx_s2(int dtype, const void* dy0, const void* wp, int kp, int b, int h, int w, float* dx, frhip_stream_t stream);

/* ---- per-step operand preparation of ALL conv weights in one launch (the reference casts them implicitly under autocast,
 * nets/resnet.py:23-46 + model/FR_PartialFC.py:166-170).  Per tensor w[k][rs][c] fp32: wc[k][rs][c] (forward operand) and
 * wt[c][rs][k] (data-gradient operand) in `dtype`; either destination may be NULL.  tile_begin = number of 32x32 tiles
 * (ceil(k/32)*ceil(c/32)*rs per tensor) of the tensors before this one; ntiles = the total.  Table in device memory. */
typedef struct { const float* w; void* wc; void* wt; int32_t k, rs, c, tile_begin; } frhip_wprep;
int frhip_prep_conv_weights(int dtype, const frhip_wprep* table, int ntensors, int ntiles, frhip_stream_t stream);

/* Dropout mask of the backbone tails (nn.Dropout() before fc: nets/SwinV2.py:559, nets/AlterNet_SwinV2_FAN.py:743): mask[i] = 1/keep
 * with probability keep, else 0, in `dtype`; Philox-4x32-10, key = seed, counter = i / 4 (same seed -> same mask).  The caller draws
 * the seed from torch's generator, so torch.manual_seed still pins a run */
int frhip_dropout_mask(int dtype, void* mask, size_t n, float keep, long long seed, frhip_stream_t stream);

/* ---- device input pipeline: Resize -> HorizontalFlip -> Normalize(0.5,0.5) -> CoarseDropout -> CHW fp32 of the reference's
 * albumentations chain (utils/data_partial.py:134-164) in one kernel.  in: uint8 [b,hin,win,3] (HWC, device);
 * out: fp32 [b,3,size,size]; flip: int32 [b] (may be NULL); holes: int32 [b][nholes][4] = x1,y1,x2,y2 in output
 * coordinates, exclusive upper bounds, x2 <= x1 marks an unused slot (may be NULL when nholes == 0).  Dropped pixels are 0
 * (CoarseDropout fill_value 0 after Normalize).  Resize = OpenCV INTER_LINEAR (8-bit fixed point), identity when sizes match. */
int frhip_augment_u8(const uint8_t* in, float* out, const int32_t* flip, const int32_t* holes, int nholes,
                     int b, int hin, int win, int size, frhip_stream_t stream);
/* the same with RandomGamma in front (utils/data_partial.py:137-138): lut uint8 [b][256] (may be NULL), the per-image table
 * ((i / 255) ** gamma * 255 truncated to uint8, gamma = uniform(gamma_limit) / 100) applied to the source bytes before Resize */
int frhip_augment_u8_lut(const uint8_t* in, const uint8_t* lut, float* out, const int32_t* flip, const int32_t* holes,
                         int nholes, int b, int hin, int win, int size, frhip_stream_t stream);
/* alb.MotionBlur of the chain (utils/data_partial.py:139-140) on the uint8 HWC batch, before Resize: out = cv2.filter2D(in, -1,
 * kernel) per image -- correlation, anchor at the centre, BORDER_REFLECT_101, float accumulation, round-half-even + saturate.
 * kernels float [b][7][7]: the k x k line kernel (k = ksize[n] in {3, 5, 7}) zero-padded with its centre at (3, 3); ksize int32 [b],
 * 0 = image copied (ksize NULL: all copied).  lut (may be NULL): RandomGamma tables applied to the source bytes first.
 * out must not alias in. */
int frhip_motion_blur_u8(const uint8_t* in, uint8_t* out, const uint8_t* lut, const float* kernels, const int32_t* ksize,
                         int b, int h, int w, frhip_stream_t stream);
/* alb.ISONoise of the chain (utils/data_partial.py:142-143; albumentations functional.iso_noise) on the uint8 HWC batch:
 * RGB/255 -> HLS; hue += N(0, color_shift * 360 * intensity) wrapped to [0, 360]; L += Poisson(std(L) * intensity * 255) / 255 * (1 - L);
 * -> RGB * 255 truncated to uint8.  params float [b][2] = (color_shift, intensity), intensity <= 0: image copied.
 * Draws: lum_noise int32 [b][h][w] + color_noise float [b][h][w] (already scaled) when given (tests), else generated on the device
 * from seeds uint64 [b] (Philox-4x32-10, counter = pixel).  scratch: frhip_iso_noise_scratch_doubles(b) doubles. */
int frhip_iso_noise_scratch_doubles(int b);
int frhip_iso_noise_u8(const uint8_t* in, uint8_t* out, double* scratch, const float* params, const int32_t* lum_noise,
                       const float* color_noise, const uint64_t* seeds, int b, int h, int w, frhip_stream_t stream);

/* ---- optimizer: torch.optim.SGD(momentum, weight_decay).step() + torch.nn.utils.clip_grad_norm_ of the training step
 * (model/FR_PartialFC.py:153-160, :181-190) as multi-tensor kernels.  A chunk is a run of at most
 * FRHIP_SGD_CHUNK consecutive fp32 elements of one parameter (p), its gradient (g) and its momentum buffer (m, may be
 * NULL when momentum == 0); the chunk table lives in device memory, the (<= 8) parameter groups are passed by value.
 * d = g*coef + weight_decay*p;  m = momentum*m + d;  p -= lr*m   with coef = *clip_coef for groups with clip != 0. */
#define FRHIP_SGD_CHUNK 65536
#define FRHIP_SGD_MAX_GROUPS 8
typedef struct { float lr, weight_decay, momentum, clip; } frhip_sgd_group;
typedef struct { float* p; const float* g; float* m; uint32_t n; uint32_t group; } frhip_sgd_chunk;
/* coef_out[0] = min(1, max_norm / (||g|| + 1e-6)) over the gradients of every group with clip != 0, coef_out[1] = ||g||;
 * partial: nchunks floats of scratch */
int frhip_sgd_clip_coef(const frhip_sgd_chunk* chunks, int nchunks, const frhip_sgd_group* groups_host, int ngroups,
                        float max_norm, float* partial, float* coef_out, frhip_stream_t stream);
int frhip_sgd_multi(const frhip_sgd_chunk* chunks, int nchunks, const frhip_sgd_group* groups_host, int ngroups,
                    const float* clip_coef, frhip_stream_t stream);

/* torch.optim.AdamW(betas, eps, weight_decay) (amsgrad off), same table scheme (model/FR_PartialFC.py:153-160 'AdamW' branch;
 * nets/PartialFC.py:235-342 swaps exp_avg / exp_avg_sq rows in and out): bc1 = 1 - beta1^step, bc2 = 1 - beta2^step of the
 * step being taken, computed by the caller per group.
 * p *= 1 - lr*wd; m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g*g; p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps) */
typedef struct { float lr, beta1, beta2, eps, weight_decay, bc1, bc2, clip; } frhip_adamw_group;
typedef struct { float* p; const float* g; float* m; float* v; uint32_t n; uint32_t group; } frhip_adamw_chunk;
int frhip_adamw_clip_coef(const frhip_adamw_chunk* chunks, int nchunks, const frhip_adamw_group* groups_host, int ngroups,
                          float max_norm, float* partial, float* coef_out, frhip_stream_t stream);
int frhip_adamw_multi(const frhip_adamw_chunk* chunks, int nchunks, const frhip_adamw_group* groups_host, int ngroups,
                      const float* clip_coef, frhip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

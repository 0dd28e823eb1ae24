/* C ABI of liblarva_hip.so -- the gfx950 (MI355X) kernels behind the LarvaNet hot path.
 *
 * The reference (Geunwoo-Jeon/LarvaNet) has no FFI: its hot path is torch.nn call sites inside
 * models/LarvaNet.py / models/LarvaNetV2.py.  Every entry point below names the reference call
 * site(s) it replaces (file:line into the reference tree).  INTEGRATION.md shows the ctypes
 * binding a reference maintainer would add.
 *
 * Conventions: all tensors are contiguous fp32 NCHW device memory owned by the caller; `stream`
 * is a hipStream_t passed as void*; every call is stream-ordered, never allocates, never
 * synchronises, keeps no global mutable state (safe for hipGraph capture).  Return value: 0 on
 * success, otherwise a hipError_t code (larva_error_string() gives the text).
 */
#ifndef LARVA_HIP_H
#define LARVA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int larva_abi_version(void);
const char* larva_error_string(int code);

/* ---- weight packing ------------------------------------------------------------------------
 * nn.Conv2d weights stay in PyTorch layout [cout][cin][3][3] (models/LarvaNet.py:210,212,227,
 * 256,258; models/LarvaNetV2.py:318).  The conv kernel consumes a packed image of 8-channel K
 * chunks, [cin/8][9][8][stride(cout)]; the input-gradient pass consumes the tap-mirrored,
 * channel-transposed image [cout/8][9][8][stride(cin)]; stride(c) = c if c % 32 is 0 or 16, else c + 16 floats
 * (LDS bank layout: the 16-lane halves of a read hit rows k and k + 1).  Where c % 32 == 0 (32 and 64 channels;
 * ABI version 3: these rows used to be padded by 16 floats) the rows are unpadded and every odd row (k odd) is stored
 * with column c ^ 16 -- an opaque kernel layout: only larva_pack_weights* writes it.  cin and cout are multiples of 8.
 * larva_packed_weight_floats(cout, cin) = (cin/8) * 9 * 8 * stride(cout).
 * `w_cin_total`/`w_cin_off` select a channel slice [w_cin_off, w_cin_off+cin) of a wider weight;
 * channels >= w_cin_total pack as 0 (the 3-channel head conv is packed for a 16-channel, i.e.
 * two-chunk, zero-padded input).  Either output may be NULL. */
long long larva_packed_weight_floats(int cout, int cin);
int larva_pack_weights(const float* w, float* wpk_fwd, float* wpk_bwd, int cout, int cin,
                       int w_cin_total, int w_cin_off, void* stream);

/* njobs (<= 64) packs in ONE launch; every argument is a host array of length njobs. */
int larva_pack_weights_batch(const float* const* w, float* const* wpk_fwd, float* const* wpk_bwd,
                             const int* cout, const int* cin, const int* w_cin_total,
                             const int* w_cin_off, int njobs, void* stream);

/* Everything train_step_larva does before its first convolution, in one launch: the packed images of
 * njobs (<= 64) weights (the optimizer has just changed them, models/LarvaNet.py:114), the head's
 * input zero-padded to 16 channels (x16 [N][16][H][W]: channels [0, C) are written, the others must
 * already be zero) and the bicubic x4 base image (models/LarvaNet.py:283-285; base [N][C][4H][4W]).
 * x16 and base may be NULL (base needs x16). */
int larva_step_prologue(const float* const* w, float* const* wpk_fwd, float* const* wpk_bwd, const int* cout,
                        const int* cin, const int* w_cin_total, const int* w_cin_off, int njobs, const float* x,
                        float* x16, float* base, int N, int C, int H, int W, void* stream);

/* ---- fused 3x3 convolution (forward and input-gradient) -----------------------------------
 * Replaces nn.Conv2d(k=3,s=1,p=1) plus its elementwise neighbours:
 *   conv+ReLU                 models/LarvaNet.py:210-211, 256-257
 *   conv + torch.add(x,res)   models/LarvaNet.py:212, 217-220      (res0)
 *   ... + outer body skip     models/LarvaNet.py:246-248            (res0, res1)
 *   conv->PixelShuffle(4)->+= base   models/LarvaNet.py:258,261,263-267   (mode 1)
 *   torch.cat(features)+merge_conv   models/LarvaNetV2.py:328-330  (n_src > 1)
 * and, fed with the `wpk_bwd` image, autograd's conv input-gradient with the ReLU-backward
 * mask (mask) and the skip-connection gradient adds (res0/res1) fused.
 * src: n_src (<= 8) tensors [N][cin_per_src][H][W] (cin_per_src % 8 == 0) read as one
 * channel-concatenated input.  cout in {32, 48, 64}.
 * Epilogue order: +bias -> relu -> (mask <= 0 ? 0 : v) -> +res0 -> +res1.
 * Non-finite values follow torch: relu is `v < 0 ? 0 : v` (torch.relu: a NaN stays NaN, +Inf stays, -Inf and -0.0 give
 * what torch gives), and the mask passes v wherever !(mask <= 0) (ATen's threshold_backward: a NaN mask element passes
 * the gradient, as do +Inf and every positive value; -Inf, -0.0, +0.0 and negatives give +0.0).  bias, res0, res1 and base
 * are plain fp32 additions: a NaN or Inf in one of their elements reaches exactly that output element (that output
 * channel for bias).  A NaN or Inf activation reaches the 3 x 3 neighbourhood of its pixel in every output channel of its
 * own image and nothing else.  Every store path and tiling behaves the same.
 * mode 0: out [N][cout][H][W]; supported fusions: none | relu | mask | res0 | res0+res1.
 * mode 1: out [N][cout/16][4H][4W] = PixelShuffle(4)(conv) (+ base, same shape, may be NULL).
 * Alignment.  pitch % 4 == 0 with wpk, every src, the mode-0 out, res0, res1 and mask 16-byte aligned takes the 16-byte
 * staging path; anything else (4-byte aligned) a register-staged path with the same results bit for bit.  bias: any
 * 4-byte boundary.  mode 1 moves four HR pixels per access on every path: `out` and `base` must be 16-byte aligned
 * (hipErrorInvalidValue otherwise, from every entry point that takes a mode). */
int larva_conv3x3_fwd(const float* const* src, int n_src, int cin_per_src, const float* wpk,
                      const float* bias, const float* res0, const float* res1, const float* mask,
                      const float* base, float* out, int N, int cout, int H, int W, int relu,
                      int mode, void* stream);

/* Same, for operands whose rows are `pitch` >= W floats apart (src, res0, res1, mask, mode-0
 * out); columns [W, pitch) of the inputs must be zero and are written as zero.  Lets a width that
 * is not a multiple of 4 (DIV2K x4 LR images are 510 wide) take the 16-byte staging path. */
int larva_conv3x3_fwd_pitched(const float* const* src, int n_src, int cin_per_src, const float* wpk,
                              const float* bias, const float* res0, const float* res1, const float* mask,
                              const float* base, float* out, int N, int cout, int H, int W, int pitch,
                              int relu, int mode, void* stream);

/* njobs (2..4) independent convolutions of one shape and one fusion in ONE launch: at the training
 * shape a conv launch is one workgroup per CU, the kernel fits two, and the jobs' workgroups fill
 * each other's prologue / epilogue bubbles.  src: njobs * n_src pointers (job-major); the other
 * operands arrays of njobs pointers, or NULL when unused by all jobs.  hipErrorNotSupported (801)
 * when the 16-byte staging path does not apply: issue the jobs one by one then. */
int larva_conv3x3_fwd_batch(int njobs, const float* const* src, int n_src, int cin_per_src,
                            const float* const* wpk, const float* const* bias, const float* const* res0,
                            const float* const* res1, const float* const* mask, const float* const* base,
                            float* const* out, int N, int cout, int H, int W, int pitch, int relu, int mode,
                            void* stream);

/* LarvaHead.forward (models/LarvaNet.py:223-233: nn.Conv2d(3, 48, 3, 1, 1), no activation) as a
 * direct convolution: x [N][3][H][W] unpadded, w [cout][3][3][3] in PyTorch layout (no packed image),
 * bias [cout] or NULL, out [N][cout][H][pitch] with columns [W, pitch) zeroed; cout % 16 == 0.
 * Bandwidth-bound (0.44 MB in, 7.08 MB out at 16x3x48x48): A/B against the same layer on the MFMA
 * kernel (image zero-padded to 16 channels) in profiles/. */
int larva_head_conv3_direct(const float* x, const float* w, const float* bias, float* out, int N, int cout,
                            int H, int W, int pitch, void* stream);

/* njobs (2..4) exits of the training step, each scored by nn.L1Loss inside the conv launch
 * (models/LarvaNet.py:104-109: out_i = leg(fea_i, base); loss += L1(out_i, truth)): the image
 * PixelShuffle(4)(conv) + base is compared with `truth` in the accumulators; partial[j] receives
 * larva_exit_l1_partials(N, H, pitch) partial sums of |out - truth| (added in index order by
 * larva_loss_from_partials: reproducible), grad[j] the gradient sign(out - truth) * gval
 * (sign(0) = 0) in the pixel-unshuffled layout [N][cout][H][pitch]; out[j] ([N][cout/16][4H][4W])
 * may be NULL when the image itself is not wanted.  Replaces larva_conv3x3_fwd_batch(mode 1) +
 * larva_l1_partial_grad_batch: one launch and four 14 MB sweeps less per step.  cout 48, 16-byte
 * staging path only, and base, truth, grad and out 16-byte aligned (801 otherwise). */
int larva_exit_l1_partials(int N, int H, int pitch);
int larva_conv3x3_exit_l1_batch(int njobs, const float* const* src, int n_src, int cin_per_src,
                                const float* const* wpk, const float* const* bias, const float* const* base,
                                const float* const* truth, float* const* out, float* const* grad,
                                float* const* partial, float gval, int N, int cout, int H, int W, int pitch,
                                void* stream);

/* Strip tiles: the same convolution (bit-identical results) with the image cut into 5 x 16 and
 * 4 x 16 pixel tiles instead of 3 x 48.  Half a training batch (8 x 48 x 48) is then 256 workgroups
 * like the whole batch is with 3 x 48 tiles, so the two halves of a batch can run as two independent
 * layer chains on two streams -- two workgroups per CU, out of phase, each chain's launch boundary,
 * prologue and store burst hidden under the other's K loop (the reference's layer chain,
 * models/LarvaNet.py:205-220,236-248, has no other independent work to offer).
 * larva_strip_tile_table: host-side table of ONE H x W image's tiles (entry = y0 | x0 << 12 |
 * five_rows << 31; the two heights alternate along the table, `phase` 0 / 1 = it starts with a
 * 5-row / 4-row tile), returns the tile count (> cap: table truncated) or < 0 when H cannot be cut
 * into 5s and 4s.  larva_conv3x3_fwd_strips: larva_conv3x3_fwd_pitched with `tile_tab` = a DEVICE
 * copy of larva_strip_tile_table(H, pitch) and `tile_tab_host` = the HOST array it filled, or NULL (given, and small
 * enough -- <= 64 tiles per image, H <= 256, pitch <= 2048 --, the table travels inside the kernel arguments and a
 * workgroup finds its tile without a dependent memory round trip); plain_stores = write the output with plain instead
 * of non-temporal stores; cout 32, 48 or 64 and the 16-byte staging path only (hipErrorNotSupported otherwise).  An
 * image sub-range of a batch is addressed by offsetting the operand pointers and passing its image count as N.
 * (ABI version 5: the host table joined the signature; the `_mb` variants of version 4 are gone with the ReLU sign-bit
 * masks they carried -- built, exact and measured no faster in round 4, profiles/r04_ab_maskbits_*.txt.) */
int larva_strip_tile_table(int H, int W, int phase, unsigned* tab, int cap);
int larva_conv3x3_fwd_strips(const float* const* src, int n_src, int cin_per_src, const float* wpk,
                             const float* bias, const float* res0, const float* res1, const float* mask,
                             const float* base, float* out, int N, int cout, int H, int W, int pitch,
                             int relu, int mode, const unsigned* tile_tab, const unsigned* tile_tab_host,
                             int tiles_per_image, int plain_stores, void* stream);

/* larva_conv3x3_fwd_pitched with the tile height of the whole-tensor launch chosen by the caller.  tile_rows 0 = the
 * library's choice, as every other entry point makes it: 3 x 48-pixel tiles; 4 x 48 for 32-channel launches of more
 * tiles than the chip has workgroup slots (339 x 510: 32.9 instead of 39.1 us per layer); and a launch of more tiles
 * than slots -- a whole validation image, validate.py:94-102 -- runs as one PERSISTENT workgroup per slot that walks its
 * tiles (round 5; LARVA_PERSIST=0 in the environment: one workgroup per tile).  3 / 4 = that height (4 exists on the
 * 16-byte path at 48 / 32 channels for the epilogues of an inference forward: hipErrorNotSupported otherwise).  The
 * results do not depend on the tiling, bit for bit. */
int larva_conv3x3_fwd_tiled(const float* const* src, int n_src, int cin_per_src, const float* wpk,
                            const float* bias, const float* res0, const float* res1, const float* mask,
                            const float* base, float* out, int N, int cout, int H, int W, int pitch,
                            int relu, int mode, int tile_rows, void* stream);

/* ---- weight / bias gradient ---------------------------------------------------------------
 * Replaces autograd's conv weight/bias gradient for the call sites above (loss.backward(),
 * models/LarvaNet.py:113).  njobs (<= 64) same-shape layers per call; job i reads dy[i]
 * [N][cout][H][W] and x[i] [N][cin][H][W], uses partial[i] (larva_wgrad_partial_floats()
 * floats) as workspace and OVERWRITES dw[i] ([cout][w_cin_total[i]][3][3], channels
 * [cin_off[i], cin_off[i]+cin_valid[i])) and db[i] ([cout], may be NULL).
 * (cout, cin) in {(48,48), (48,16), (32,32), (64,64)}.  Deterministic (no atomics).
 * Alignment.  dy and x: W % 4 == 0 and 16-byte aligned pointers take 16-byte loads, anything else (4-byte aligned) a
 * narrower walk with the same results; the flat grid has only the former (hipErrorNotSupported).  partial[i] (and
 * head_partial) is written and reduced 16 bytes per lane on every path: 16-byte aligned, hipErrorInvalidValue
 * otherwise, from every entry point that takes it.  dw and db: any 4-byte boundary. */
long long larva_wgrad_partial_floats(int cout, int cin, int splits);
/* Workgroups of the (cout, cin) weight-gradient kernel that share a CU (1 or 2: the small shapes -- (32,32), the (C,16)
 * heads -- fit twice and hide each other's staging phases): launch 256 * this many workgroups in total to fill the chip. */
int larva_wgrad_cu_share(int cout, int cin);
int larva_conv3x3_wgrad(const float* const* dy, const float* const* x, float* const* partial,
                        float* const* dw, float* const* db, const int* cin_off,
                        const int* cin_valid, const int* w_cin_total, int njobs, int splits,
                        int N, int cout, int cin, int H, int W, void* stream);

/* Phase 1 as ONE grid of nwg workgroups over all njobs (<= 64) layers: their tiles form one sequence
 * cut evenly over the workgroups (no CU idles at any layer count; a workgroup whose share crosses a
 * layer boundary contributes a partial image to both layers).  48 -> 48, 32 -> 32 or 64 -> 64 channels (the last
 * as two passes over 32 input channels each per workgroup and layer), W % 4 == 0, 16-byte
 * aligned tensors (hipErrorNotSupported otherwise).  splits_out[i] = partial images of layer i for
 * larva_wgrad_reduce; partial[i] holds larva_wgrad_flat_max_splits(njobs, nwg, tiles per layer) images
 * (tiles per layer = N * ceil(H/3) * ceil(W/48)). */
int larva_wgrad_flat_max_splits(int njobs, int nwg, int tiles_per_layer);
int larva_conv3x3_wgrad_partial_flat(const float* const* dy, const float* const* x, float* const* partial,
                                     int njobs, int nwg, int N, int cout, int cin, int H, int W,
                                     int* splits_out, void* stream);
/* The same grid with LarvaHead's weight gradient (models/LarvaNet.py:227-233; a (48, 16) layer: head_x16 = the
 * head's input zero-padded to 16 channels, [N][16][H][W]) as the tail of the sequence: the last workgroups take
 * its tiles (priced at 0.7 of a 48 -> 48 tile) instead of a launch of its own behind this one.  head_partial holds
 * larva_wgrad_flat_head_splits(njobs, nwg, tiles per layer) images of larva_wgrad_partial_floats(48, 16, 1)
 * floats; *head_splits_out = the images written (what larva_wgrad_reduce needs for that layer). */
int larva_wgrad_flat_head_splits(int njobs, int nwg, int tiles_per_layer);
int larva_conv3x3_wgrad_partial_flat_head(const float* const* dy, const float* const* x, float* const* partial,
                                          int njobs, const float* head_dy, const float* head_x16, float* head_partial,
                                          int nwg, int N, int H, int W, int* splits_out, int* head_splits_out,
                                          void* stream);

/* The two phases separately: partial images for njobs (<= 64) layers, and the fixed-order
 * reduction of up to 64 layers' partial images (each with its own split count and kernel shape)
 * in one launch. */
int larva_conv3x3_wgrad_partial(const float* const* dy, const float* const* x, float* const* partial,
                                int njobs, int splits, int N, int cout, int cin, int H, int W,
                                int* splits_used, void* stream);
int larva_wgrad_reduce(const float* const* partial, float* const* dw, float* const* db,
                       const int* cin_off, const int* cin_valid, const int* w_cin_total,
                       const int* splits, const int* cout, const int* cin, int njobs, void* stream);

/* larva_wgrad_reduce + larva_loss_from_partials in ONE launch (same arguments, same arithmetic as the two):
 * the loss of a training step (models/LarvaNet.py:104-109) is not needed before the step ends, so its
 * finishing block rides on the last launch of backward. */
int larva_wgrad_reduce_with_loss(const float* const* partial, float* const* dw, float* const* db,
                                 const int* cin_off, const int* cin_valid, const int* w_cin_total,
                                 const int* splits, const int* cout, const int* cin, int njobs,
                                 const float* const* terms, const int* count, const float* scale, int nterms,
                                 float divisor, float* loss_out, void* stream);

/* ---- base image -----------------------------------------------------------------------------
 * F.interpolate(x, scale_factor=4, mode='bicubic', align_corners=False), models/LarvaNet.py:283-285.
 * in [N][C][H][W] -> out [N][C][4H][4W].  An `out` that is not 16-byte aligned is written with 4-byte stores (the same
 * values bit for bit). */
int larva_bicubic4_fwd(const float* in, float* out, int N, int C, int H, int W, void* stream);
/* F.interpolate(x, scale_factor=4, mode, align_corners=False) for the modes with which the reference's call
 * (models/LarvaNet.py:57,283-285) does not raise: mode 0 bicubic (as above), 1 bilinear.  out 16-byte aligned. */
int larva_upsample4_fwd(const float* in, float* out, int N, int C, int H, int W, int mode, void* stream);

/* ---- L1 loss ---------------------------------------------------------------------------------
 * nn.L1Loss() forward/backward, models/LarvaNet.py:85,108,113.  Pointers 16-byte aligned. */
int larva_l1_workspace_floats(void);
int larva_l1_fwd(const float* a, const float* b, long long numel, float* partial, float* loss,
                 void* stream);
int larva_l1_bwd(const float* a, const float* b, const float* gout, long long numel, float* ga,
                 void* stream);
/* nn.L1Loss backward fused with the nn.PixelShuffle(4) backward of the exit it scores
 * (models/LarvaNet.py:108,113,261): a, b [N][C][4H][4W] -> ga [N][16C][H][W]. */
/* ga = sign(a - b) * (gout[0] * gscale) / numel; gscale carries the 1/num_modules of the mean over
 * exits (models/LarvaNet.py:109) so that no separate scaling pass is needed. */
int larva_l1_bwd_unshuffle4(const float* a, const float* b, const float* gout, float gscale, float* ga, int N,
                            int C, int H, int W, void* stream);
/* `loss += ...; loss / num_modules` (models/LarvaNet.py:104-109): out = (sum of n <= 8 device scalars) / divisor. */
int larva_sum_scalars(const float* const* terms, int n, float divisor, float* out, void* stream);
/* The same loss tail in two launches less per exit: larva_l1_partial leaves the block partial sums
 * of sum|a - b| (*blocks <= larva_l1_workspace_floats() floats), larva_loss_from_partials computes
 * ( sum_i scale[i] * sum(terms[i][0..count[i])) ) / divisor for n <= 8 terms (scale = 1 / numel for
 * partial sums; count 1, scale 1 for a ready scalar) -- bit-identical to larva_l1_fwd per exit
 * followed by larva_sum_scalars. */
int larva_l1_partial(const float* a, const float* b, long long numel, float* partial, int* blocks_out,
                     void* stream);
int larva_loss_from_partials(const float* const* terms, const int* count, const float* scale, int n,
                             float divisor, float* out, void* stream);
/* `return loss.item()` (models/LarvaNet.py:139) without waiting for the rest of the step: larva_host_cell_alloc
 * hands out 8 bytes {float value; uint32 sequence} of coherent, device-mapped pinned host memory (NaN, 0 on return);
 * the _to_host variant stores the loss there as well, together with sequence + 1, as ONE system-scope 8-byte release
 * store, and the host polls the cell instead of synchronising: it counts its launches and takes the value once the
 * sequence number is its own count (a late store of an earlier launch cannot be mistaken for this one's).
 * host_cell may be NULL (= larva_loss_from_partials).  larva_host_cell_free waits for the device before it frees. */
int larva_loss_from_partials_to_host(const float* const* terms, const int* count, const float* scale, int n,
                                     float divisor, float* out, float* host_cell, void* stream);
/* ... _seq: the same with the cell's sequence number ALSO kept in device memory (`dev_seq`, one zero-initialised
 * unsigned owned by the caller, used by no other cell): the launch takes the number from there instead of reading the
 * host cell back over PCIe before it can store (NULL = larva_loss_from_partials_to_host). */
int larva_loss_from_partials_to_host_seq(const float* const* terms, const int* count, const float* scale, int n,
                                         float divisor, float* out, float* host_cell, unsigned* dev_seq, void* stream);
int larva_host_cell_alloc(float** cell);
int larva_host_cell_free(float* cell);
/* larva_l1_partial and larva_l1_bwd_unshuffle4 in one pass over (a, b), for a gradient value known
 * on the host (training seeds loss.backward() with 1): grad [N][16C][H][W] = sign(a - b) * gvalue *
 * gscale / numel, a, b [N][C][4H][4W]; same partial sums and gradient values as the two calls. */
int larva_l1_partial_grad(const float* a, const float* b, float gvalue, float gscale, float* partial,
                          int* blocks_out, float* grad, int N, int C, int H, int W, void* stream);
/* The same for n <= 8 exit images a[i] scored against one truth image b, in one launch. */
int larva_l1_partial_grad_batch(const float* const* a, const float* b, int n, float gvalue, float gscale,
                                float* const* partial, int* blocks_out, float* const* grad, int N, int C, int H,
                                int W, void* stream);

/* ---- PixelShuffle(4) backward (models/LarvaNet.py:261): in [N][C][4H][4W] -> out [N][16C][H][W]; `in` 16-byte aligned
 * (hipErrorInvalidValue otherwise) */
int larva_pixel_unshuffle4(const float* in, float* out, int N, int C, int H, int W, void* stream);

/* ---- x2 / x3 (csrc/larva_scale.hip) ---------------------------------------------------------
 * A network prepared with scales=[s], s = 2 or 3: the last conv of every leg (and of the V2 tail) has C s^2 outputs
 * (C = 3: 12 / 27), run as a plain 32-output conv on zero-padded weights; its output / gradient is [N][cpad][H][*]
 * with cpad >= C s^2, channel c s^2 + i s + j = colour c, sub-pixel (i, j).  Gradient outputs write channels
 * [C s^2, cpad) as zeros.
 * F.interpolate(x, scale_factor=scale, mode, align_corners=False), mode 0 bicubic / 1 bilinear, scale 2, 3 or 4 (4 =
 * larva_upsample4_fwd): in [N][C][H][W] -> out [N][C][scale H][scale W]. */
int larva_upsample_fwd(const float* in, float* out, int N, int C, int H, int W, int scale, int mode, void* stream);
/* out [N][C][scale H][scale W] = PixelShuffle(scale)(y) + base (base may be NULL); y [N][cpad][H][pitch] (0 = W). */
int larva_pixel_shuffle_base(const float* y, const float* base, float* out, int N, int C, int cpad, int H, int W,
                             int pitch, int scale, void* stream);
/* PixelShuffle(scale) backward: in [N][C][scale H][scale W] -> out [N][cpad][H][W]. */
int larva_pixel_unshuffle(const float* in, float* out, int N, int C, int cpad, int H, int W, int scale, void* stream);
/* L1 backward in that layout: ga [N][cpad][H][W] = sign(a - b) * (gout[0] * gscale) / numel. */
int larva_l1_bwd_unshuffle(const float* a, const float* b, const float* gout, float gscale, float* ga, int N, int C,
                           int cpad, int H, int W, int scale, void* stream);
/* One training exit after its plain conv y [N][cpad][H][W], in one pass: out = PixelShuffle(scale)(y) + base (out may be
 * NULL), *blocks_out <= larva_l1_workspace_floats() block partial sums of sum|out - truth| into `partial` (for
 * larva_loss_from_partials, scale 1 / numel) and grad [N][cpad][H][W] = sign(out - truth) * gvalue * gscale / numel. */
int larva_shuffle_l1_partial_grad(const float* y, const float* base, const float* truth, float gvalue, float gscale,
                                  float* partial, int* blocks_out, float* grad, float* out, int N, int C, int cpad, int H,
                                  int W, int scale, void* stream);

/* ---- AdamW over a flat buffer (optim.AdamW, models/LarvaNet.py:86-88,114) ------------------
 * step_lr: device floats {step (1-based), lr}.  g is multiplied by grad_scale first
 * (1/world_size after a sum all-reduce).  Buffers that are all 16-byte aligned are walked 16 bytes per lane
 * (any n; the tail is element-wise), others element-wise; the values are the same either way. */
int larva_adamw_step(float* p, const float* g, float* m, float* v, const float* step_lr,
                     double beta1, double beta2, double eps, double weight_decay, float grad_scale,
                     long long n, void* stream);

/* The same update with step (1-based) and lr from the host.  The hyper-parameters are DOUBLES, as torch.optim.AdamW's
 * are (Python floats): 1 - beta^step, lr / (1 - beta1^step), 1 - lr * weight_decay, 1 - beta1 and 1 - beta2 are
 * computed in double and rounded to float once, exactly the scalars ATen's kernels receive (in float arithmetic
 * 1.f - 0.999f is 0.00100004673, not 0.001f).  The kernel follows torch's single-tensor step operation by operation:
 * against torch 2.10 on the CPU the moments are bit-identical, the parameters on all but ~0.1 % of the elements (1 ulp). */
int larva_adamw_step_host(float* p, const float* g, float* m, float* v, int step, double lr, double beta1,
                          double beta2, double eps, double weight_decay, float grad_scale, long long n,
                          void* stream);
/* larva_adamw_step_host that also copies one float, copy_dst[0] = copy_src[0] (both may be NULL): the step's
 * loss out of the captured graph's static buffer into a tensor the caller keeps (models/LarvaNet.py:139). */
int larva_adamw_step_host_copy(float* p, const float* g, float* m, float* v, int step, double lr, double beta1,
                               double beta2, double eps, double weight_decay, float grad_scale, long long n,
                               const float* copy_src, float* copy_dst, void* stream);

/* ---- device-resident patch sampler ----------------------------------------------------------
 * Crop + np.rot90(k) + horizontal flip + uint8->float of a training batch from a dataset held
 * in HBM (dataloaders/div2k_train_loader.py:72-98 and the H2D copy of train_larva.py:123-124).
 * data: uint8 CHW images at data + offsets[i], (H, W) = hw[2i], hw[2i+1]; draws[b] =
 * {image, x, y, k, flip}; crop origin (y*mult, x*mult), size P x P; out [B][3][P][P] float. */
int larva_gather_patches(const unsigned char* data, const long long* offsets, const int* hw,
                         const int* draws, float* out, int B, int P, int mult, void* stream);

/* ---- validation metric on the device (validate.py:17-27) --------------------------------------
 * acc[0] += sum (truth_u8 - clip(rint(out), 0, 255))^2 over out [C][H][W] float against truth
 * [C][TH][TW] uint8 cropped top-left; exact integer.  Caller zeroes acc. */
int larva_sqerr_u8(const float* out, const unsigned char* truth, int C, int H, int W, int TH, int TW,
                   unsigned long long* acc, void* stream);

/* ---- 8-bit images (uint8 in, uint8 out) --------------------------------------------------------
 * larva_u8_hwc_to_f32_chw: in uint8 [N][H][W][3] (a decoded PNG) -> out float [N][3][H][W], exact.
 * larva_f32_chw_to_u8_hwc: in float [N][3][H][W] -> out uint8 [N][H][W][3], q = min(max(rint(v), 0), 255): round half to
 * even, then clamp -- larva_sqerr_u8's arithmetic, numpy's clip(round(v), 0, 255) for every finite v (and for +-inf);
 * a NaN becomes 0.  Any N, H, W >= 1.  Where H W is a multiple of 4 and both pointers are 16-byte aligned a lane moves
 * 4 pixels (16-byte accesses per colour plane, 12 contiguous bytes of the uint8 image), otherwise one; the values do not
 * depend on the path. */
int larva_u8_hwc_to_f32_chw(const unsigned char* in, float* out, int N, int H, int W, void* stream);
int larva_f32_chw_to_u8_hwc(const float* in, unsigned char* out, int N, int H, int W, void* stream);

/* ---- benchmark metrics of two uint8 HWC images (csrc/larva_metrics.hip) ------------------------------
 * out, truth: uint8 [rows][pitch bytes], pixel (y, x) at y * pitch + 3 x.  The window is rows [y0, y0 + h) and columns
 * [x0, x0 + w) of BOTH images (1 <= h, w <= 32768; pitch >= 3 (x0 + w); the caller guarantees the rows exist).  mode 0:
 * the three colour planes; mode 1: the BT.601 luma plane, Y = 16 + round_half_even((65481 R + 128553 G + 24966 B) /
 * 255000) in integers.  result (8 x 8 bytes, device memory, written by a final one-workgroup launch):
 *   [0] uint64  sum of squared differences over the window and the mode's planes (exact)
 *   [1..3] double  sum of the SSIM samples per plane (0 for unused planes or want_ssim == 0)
 *   [4] int64  SSIM samples per plane = (h - 10) (w - 10), 0 without SSIM   [5] int64 h w planes   [6] int64 planes
 * SSIM: 11-tap normalised Gaussian (sigma 1.5) over x, y, x^2, y^2, x y in double, K1 0.01, K2 0.03, range 255,
 * population covariance, samples = the window minus 5 pixels on every side (needs h, w >= 11).  All sums are taken in a
 * fixed order: results are bitwise reproducible.  workspace: larva_u8_metrics_workspace_bytes(h, w, mode) bytes,
 * 8-byte aligned, the caller's; nothing is allocated or synchronised. */
long long larva_u8_metrics_workspace_bytes(int h, int w, int mode);
int larva_u8_metrics(const unsigned char* out, long long out_pitch, const unsigned char* truth, long long truth_pitch,
                     int y0, int x0, int h, int w, int mode, int want_ssim, void* workspace,
                     unsigned long long* result, void* stream);

/* ---- fp16 inference (--precision fp16; csrc/conv3x3_f16.hip) -------------------------------------
 * Grad-free x4 forward at 48 channels on v_mfma_f32_16x16x32_f16: fp16 storage, fp32 accumulation.  fp16 tensors are
 * uint16_t bit images of IEEE half, CHANNELS-LAST [N][H][W][48] (not the fp32 NCHW of the entry points above); images
 * and bases stay fp32 NCHW.  `flag` is one device unsigned that an fp16-storing launch sets to 1 (never clears) when a
 * value is not finite or exceeds 65504 in magnitude before it is rounded; the caller zeroes it.
 * Alignment (there is no narrower walk: hipErrorInvalidValue before any launch otherwise).  16 bytes: every fp16
 * activation (srcs, res0, res1, out, the head's out), every packed weight image, the fp32 bias of the conv entry points,
 * the fp32 base and fp32 HR out.  4 bytes: the uint8 HR out.  Any boundary their type allows: the head's x, w and bias,
 * the fp32 weight larva_f16_pack_weights reads, and flag.
 *
 * larva_f16_packed_weight_halves(48, 48 m) = m * 14 * 3 * 64 * 8 (m <= 8; -1 for any other shape): the A-operand image of
 * a [48][48 m][3][3] fp32 weight, [src m][K-step 14][M tile 3][lane 64][8] halves, K = (tap, 8-channel group), rounded to
 * nearest even; larva_f16_pack_weights writes it in one launch. */
long long larva_f16_packed_weight_halves(int cout, int cin);
int larva_f16_pack_weights(const float* w, uint16_t* wpk, int cout, int cin, void* stream);

/* Head conv (models/LarvaNet.py:227): x fp32 [N][3][H][W] -> out fp16 [N][H][W][48] = conv(x, w) + bias, w the fp32
 * [48][3][3][3] parameter itself.  fp32 operands and an fp32 fmaf chain (VALU), then one rounding to fp16. */
int larva_f16_head(const float* x, const float* w, const float* bias, uint16_t* out, unsigned* flag, int N, int H,
                   int W, void* stream);

/* 48 -> 48 conv over nsrc (1..8) fp16 inputs read as consecutive 48-channel K chunks (the V2 merge conv over the body
 * outputs without a concatenation, models/LarvaNetV2.py:330), wpk packed for cin = 48 nsrc.  Epilogue in fp32:
 * + bias, then ReLU (relu != 0; models/LarvaNet.py:210-212,256) or + res0 (+ res1: the body's outer skip,
 * models/LarvaNet.py:219,247), rounded once to fp16.  relu excludes res0; res1 needs res0.  srcs is a host array. */
int larva_f16_conv3x3(const uint16_t* const* srcs, int nsrc, const uint16_t* wpk, const float* bias,
                      const uint16_t* res0, const uint16_t* res1, int relu, uint16_t* out, unsigned* flag, int N, int H,
                      int W, void* stream);

/* Leg end (models/LarvaNet.py:258-265): out fp32 [N][3][4H][4W] = PixelShuffle(4)(conv(src) + bias) + base, base the
 * fp32 x4 base image (larva_upsample4_fwd). */
int larva_f16_conv3x3_shuffle_base(const uint16_t* src, const uint16_t* wpk, const float* bias, const float* base,
                                   float* out, int N, int H, int W, void* stream);

/* The same leg end as a uint8 image: out uint8 [N][4H][4W][3] = larva_f32_chw_to_u8_hwc of what
 * larva_f16_conv3x3_shuffle_base stores, bit for bit, without the fp32 HR image ever reaching memory.  Sets *flag when a
 * value it quantises is not finite. */
int larva_f16_conv3x3_shuffle_base_u8(const uint16_t* src, const uint16_t* wpk, const float* bias, const float* base,
                                      unsigned char* out, unsigned* flag, int N, int H, int W, void* stream);

/* Job launches: njobs (1..8) independent single-source 48 -> 48 convs of ONE shape in one grid -- the legs of a multi-exit
 * network once the bodies have run.  srcs, wpks, biases and outs are host arrays of njobs device pointers (job j reads
 * srcs[j], wpks[j], biases[j] and writes outs[j]); every pointer must be non-NULL.  Job j stores bit for bit what the
 * single-job entry point stores for its operands: a workgroup runs the same tile code after looking its job up from its
 * block index.  larva_f16_conv3x3_jobs: + bias, then ReLU if relu != 0, rounded once to fp16 (larva_f16_conv3x3 with one
 * source and no residual): the legs' first conv. */
int larva_f16_conv3x3_jobs(int njobs, const uint16_t* const* srcs, const uint16_t* const* wpks,
                           const float* const* biases, int relu, uint16_t* const* outs, unsigned* flag, int N, int H,
                           int W, void* stream);

/* The leg end of every job against ONE shared fp32 base image [N][3][4H][4W]: exactly one of outs_f32 (njobs fp32
 * [N][3][4H][4W] images, larva_f16_conv3x3_shuffle_base per job) and outs_u8 (njobs uint8 [N][4H][4W][3] images,
 * larva_f16_conv3x3_shuffle_base_u8 per job; needs flag) is given, the other is NULL.  Both job entry points return
 * hipErrorInvalidValue before any launch for njobs outside 1..8, a NULL pointer in an array, both or neither output
 * array, or a shape whose grid (njobs times the tiles rounded up to a multiple of 8) does not fit. */
int larva_f16_conv3x3_shuffle_base_jobs(int njobs, const uint16_t* const* srcs, const uint16_t* const* wpks,
                                        const float* const* biases, const float* base, float* const* outs_f32,
                                        unsigned char* const* outs_u8, unsigned* flag, int N, int H, int W,
                                        void* stream);

/* ---- geometric self-ensemble (--self_ensemble; csrc/larva_ensemble.hip) ------------------------------
 * dihedral(a, t), t = 0..7, over the spatial axes: reverse rows if t & 1, then reverse columns if t & 2, then swap the axes
 * if t & 4 (image_utils.dihedral).  larva_dihedral_inputs_u8 / _f32: in uint8 [N][H][W][3] / float [N][3][H][W] -> the
 * eight images as batch slots of two fp32 NCHW tensors, exact: image n under t in slot 4 n + t of a [4N][3][H][W] for
 * t < 4 and in slot 4 n + t - 4 of b [4N][3][W][H] for t >= 4.  One launch; each source pixel is read once.
 *
 * larva_dihedral_mean: a [4N][3][H][W] and b [4N][3][W][H] (the forward's outputs: H, W are the HR sizes here), v_t =
 * dihedral_inv(slot t) -> E = (((((((v0 + v1) + v2) + v3) + v4) + v5) + v6) + v7) * 0.125f per pixel, fp32 adds in this
 * order whatever the tile, into out_f32 [N][3][H][W] or, quantised as larva_f32_chw_to_u8_hwc does, into out_u8
 * [N][H][W][3]; exactly one of the two is given, the other NULL.  One launch, no intermediate image; b is read through
 * an LDS transpose.  Any N, H, W >= 1; 16-byte accesses where H and W are multiples of 4 and the pointers aligned, the
 * values do not depend on the path. */
int larva_dihedral_inputs_u8(const unsigned char* in, float* a, float* b, int N, int H, int W, void* stream);
int larva_dihedral_inputs_f32(const float* in, float* a, float* b, int N, int H, int W, void* stream);
int larva_dihedral_mean(const float* a, const float* b, float* out_f32, unsigned char* out_u8, int N, int H, int W,
                        void* stream);

/* ---- bicubic decimation of uint8 images (csrc/larva_downscale.hip) -------------------------------------
 * The degradation SR inputs are made with: antialiased bicubic decimation by s = 2, 3 or 4 in the MATLAB imresize
 * convention, exact in integers.  Output h = H / s, w = W / s (floor, both >= 1); only the top-left h s x w s pixels are
 * read.  Along an axis output i takes inputs j = s i + o with integer weights over D,
 *   s = 2: D = 256,  o = -3..4:  -3 -9 29 111 111 29 -9 -3
 *   s = 3: D = 81,   o = -4..6:  -1 -2 0 9 21 27 21 9 0 -2 -1
 *   s = 4: D = 4096, o = -6..9:  -7 -45 -75 -49 93 399 745 987 987 745 399 93 -49 -75 -45 -7
 * (the Keys cubic, a = -1/2, c((u - j) / s) / s at u = (i + 1/2) s - 1/2); j outside [0, n), n the cropped length, reflects:
 * m = j mod 2 n, j' = m < n ? m : 2 n - 1 - m.  out = clip(round_half_even(N / D^2), 0, 255), N the exact integer double
 * sum: one rounding, at the end.  image_utils.bicubic_downscale_u8 is the same on the host, byte for byte.
 *
 * larva_bicubic_down_u8: one image, src uint8 HWC with `pitch` >= 3 W bytes per row (any pitch and any alignment: a
 * window into a larger image), dst uint8 [h][w][3] contiguous.  One launch.
 *
 * larva_bicubic_down_u8_table: n images of a byte table in ONE launch.  Image i is at data + offsets[i] with (H, W) =
 * hw[2 i], hw[2 i + 1] (device arrays, as larva_gather_patches takes them) and goes to out + out_offsets[i]; planar == 0:
 * HWC images [H][W][3] -> [h][w][3]; planar != 0: CHW images [3][H][W] (the sampler's tables) -> [3][h][w], every plane
 * an image of its own.  The grid is flat: tile_prefix (device, int [n + 1]) holds the workgroups of the images before i,
 * image i having planes * ceil(h / 8) * ceil(w / (planar ? 96 : 32)) of them (planes = planar ? 3 : 1), and total_tiles =
 * tile_prefix[n].  Bytes of `out` outside the images are not touched. */
int larva_bicubic_down_u8(const unsigned char* src, int H, int W, long long pitch, int s, unsigned char* dst,
                          void* stream);
int larva_bicubic_down_u8_table(const unsigned char* data, const long long* offsets, const int* hw, int n, int s,
                                int planar, unsigned char* out, const long long* out_offsets, const int* tile_prefix,
                                int total_tiles, void* stream);

/* ---- planar YUV 4:2:0 video frames (csrc/larva_yuv.hip) -----------------------------------------------
 * An I420 frame of W x H luma pixels is one buffer: Y [H][W], then U [ch][cw], then V [ch][cw], cw = (W + 1) / 2,
 * ch = (H + 1) / 2 (odd W, H are legal); frame n of a batch of N frames of one size starts at n * frame_pitch_bytes
 * (>= the frame's bytes).  Chroma is centred on 128 and sited in the centre of its 2 x 2 luma block; a coordinate outside a
 * plane is clamped to the edge.  Both conversions are exact int32 arithmetic, defined by image_utils.i420_to_rgb_f32 /
 * rgb_u8_to_i420 and equal to them bit for bit; the matrix (BT.601 / BT.709) and the range (limited / full) are in
 * coef_table, a HOST array read during the call (image_utils.yuv_to_rgb_table / rgb_to_yuv_table build it).
 *
 * larva_i420_to_rgb_f32: coef_table = int[6] {luma offset, cy, crv, cgu, cgv, cbu}, the inverse-matrix entries * 4096.
 * out fp32 [N][3][H][W], values on [0, 255] in steps of 1 / 256: with u, v = the chroma planes filtered to the luma grid
 * (9 3 3 1 towards the nearer neighbours, * 16, - 2048) and L = (Y - offset) 16 cy, R = L + crv v, G = L + cgu u + cgv v,
 * B = L + cbu u, value = clamp((sum + 128) >> 8, 0, 65280) / 256.
 *
 * larva_rgb_u8_to_i420: img uint8 [N][H][W][3] -> N frames.  coef_table = int[10] {luma offset, Y row, U row, V row}, the
 * forward-matrix rows * 65536 (|row| sums <= 2 * 65536): Y = clamp((row . rgb + (offset << 16) + 2^15) >> 16, 0, 255); a
 * chroma sample, S the per-channel sums of its 2 x 2 block with edge pixels repeated, = clamp((row . S + (128 << 18) +
 * 2^17) >> 18, 0, 255).  Bytes of a frame's pitch beyond the frame are not touched.
 *
 * One launch each, any N, H, W >= 1 (H, W <= 32768); hipErrorInvalidValue before the launch for a NULL pointer, a bad
 * shape, a pitch below the frame size or a table outside the bounds that keep the sums inside int32. */
int larva_i420_to_rgb_f32(const unsigned char* frames, long long frame_pitch_bytes, float* out, int N, int H, int W,
                          const int* coef_table, void* stream);
int larva_rgb_u8_to_i420(const unsigned char* img, unsigned char* out, long long frame_pitch_bytes, int N, int H, int W,
                         const int* coef_table, void* stream);

/* ---- bicubic resize of uint8 images to any size (csrc/larva_resize.hip) ----------------------------------
 * Pillow's Image.resize((w, h), Image.BICUBIC) of an RGB uint8 image, byte for byte, both passes in ONE launch, int32 only.
 * src uint8 [N][H][W][3] -> dst uint8 [N][h][w][3], both contiguous, H <= 4 h and W <= 4 w (any upsampling).  Per axis two
 * DEVICE int32 tables (image_utils.resize_coeffs makes them): bounds [n_out][2] = (lo, n) and coeffs [n_out][ksize], ksize =
 * 2 ceil(2 max(n_in / n_out, 1)) + 1 <= 17; one pass is out[i] = clamp((2^21 + sum_{j < n} in[lo + j] coeffs[i][j]) >> 22, 0,
 * 255) (arithmetic shift).  The horizontal pass (hbounds, hcoeffs, kx) runs first and leaves bytes, then the vertical one
 * (vbounds, vcoeffs, ky).  An axis whose size does not change passes ksize 0 and NULL tables and is copied.
 * hipErrorInvalidValue before the launch for a NULL pointer, a size below 1 or above 2^20, N above 65535, a ratio above 4,
 * a ksize that is not the one of the axis' ratio, or more than 65535 * 16 output rows. */
int larva_resize_u8(const unsigned char* src, unsigned char* dst, int N, int H, int W, int h, int w, const int* hbounds,
                    const int* hcoeffs, int kx, const int* vbounds, const int* vcoeffs, int ky, void* stream);

/* ---- transparency: straight-alpha RGBA images (csrc/larva_rgba.hip) --------------------------------------
 * An RGBA batch runs through the RGB forward as N + K batch slots: slot n is image n's colour, and an image that is not
 * opaque owns one more slot, alpha_slot[n] in [N, N + K), that carries its alpha plane as a grey image.  alpha_slot is a
 * DEVICE int32 [N] (image_utils.alpha_slots makes it; K <= N); an entry outside [N, N + K) -- -1 by convention -- marks an
 * opaque image, so no entry can send an access outside the tensors.  image_utils.rgba_split_f32 / rgba_merge_u8 are the
 * definition and both launches equal them bit for bit.
 *
 * larva_rgba_u8_split_f32: rgba uint8 [N][H][W][4] -> out fp32 [N + K][3][H][W], exact: out[n][c] = channel c of image
 * n, out[alpha_slot[n]][0..2] = its alpha.  Slots no image names are not written.
 * larva_rgb_u8_merge_rgba: rgb uint8 [N + K][h][w][3] -> out uint8 [N][h][w][4]: channels 0..2 from slot n, channel 3 =
 * (r + g + b + 1) / 3 of slot alpha_slot[n] in integers, 255 for an opaque image.
 *
 * One launch each, any N, H, W >= 1.  Where H W is a multiple of 4 and the pointers are aligned (RGBA images and fp32
 * planes to 16 bytes, RGB images to 4) a lane moves 4 pixels with 16-byte accesses to the RGBA image and the planes;
 * otherwise one pixel per lane, the RGBA pixel as one word where that image is 4-byte aligned, else as bytes.  The values
 * do not depend on the path.  hipErrorInvalidValue before the launch for a NULL pointer or a bad shape. */
int larva_rgba_u8_split_f32(const unsigned char* rgba, const int* alpha_slot, float* out, int N, int K, int H, int W,
                            void* stream);
int larva_rgb_u8_merge_rgba(const unsigned char* rgb, const int* alpha_slot, unsigned char* out, int N, int K, int h, int w,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LARVA_HIP_H */

/* nerf_hip.h -- C ABI of libnerf_hip.so, the MI355X (gfx950) implementation of the
 * nerf-pytorch volumetric-rendering hot path.
 *
 * The reference (yenchenlin/nerf-pytorch) is pure Python and has no FFI: the seam this
 * library plugs into is the call surface of its hot-path functions.  Every entry point
 * below names the reference function (file:line under /root/reference) it replaces.
 * A maintainer binds these with ctypes (INTEGRATION.md shows the stub); the in-repo
 * binding is nerf-pytorch_amd/hip_backend.py.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 data owned by the caller (torch tensors);
 *     the library allocates nothing and keeps no pointer after return;
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream); all work is
 *     enqueued asynchronously on it, no host synchronisation inside;
 *   - return 0 on success, a negative NERF_E_* code for argument errors, a positive
 *     hipError_t for runtime errors; nerf_last_error() describes the last failure of the
 *     calling thread.  Nothing throws, nothing exits;
 *   - rays are [n_rays][ray_stride] records (o3, d3, near, far, viewdir3), ray_stride = 11
 *     (run_nerf.py:117-123);
 *   - the field model is fixed to the reference architecture NeRF(D=8, W=256,
 *     input_ch=63, input_ch_views=27, skips=[4], use_viewdirs=True)
 *     (run_nerf_helpers.py:67-94); parameters are exchanged as ONE flat fp32 vector in
 *     state_dict order (nerf_param_count() = 595,844 floats, layout: nerf_param_offset()).
 */
#ifndef NERF_HIP_H
#define NERF_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define NERF_ABI_VERSION 10
#define NERF_E_BADARG (-1)      /* null pointer / non-positive size / unsupported shape */
#define NERF_E_UNSUPPORTED (-2) /* configuration outside the fixed architecture */

/* ---- THE DATAPATH TABLE.  Everything below runs on one of four training datapaths, plus one inference form of the third.  Each
 * family of entry points names them by an integer code of its own; this is every code there is ("-": the family has no such form).
 *
 *                          fp32          bf16x3        fp16x3        fp16x3w            fp16_fp8c (inference form of fp16x3)
 *   products               exact fp32    3 x bf16      3 x fp16      3 x fp16           fp16 main + 2 x fp8 corrections
 *   `split`   forward      - (a)         0             1             5 (b)              2, 3 = last sample left out; act NULL
 *             dgrad        - (a)         0             1             5                  -
 *             repack       - (a)         0             1             1                  2 (nerf_pack_params_split only)
 *   `datapath` wgrad (c)   0             4             5             6                  -
 *   `datapath` sizes (d)   0             1             1             2                  -
 *   `family`   layout (d)  0             1             1             2                  -
 *   NerfRenderCfg.precision 0            1             3             5                  -
 *   act kind    (e)        0             4             5             6                  -
 *   delta kind  (e)        0             2             3             4                  -
 *
 *   (a) the entry points without `split`: nerf_pack_params, nerf_field_fwd, nerf_field_bwd / _dgrad / _wgrad
 *   (b) with act = NULL the launch is split 1's
 *   (c) nerf_field_wgrad_phase[_live]; -1 = as recorded for the act / delta pair
 *   (d) nerf_*_floats_dp, nerf_debug_layout: 0 fp32 rows, 1 tiles of 16-bit elements, 2 hi + lo tiles (two-word saves)
 *   (e) what nerf_buffer_layout returns for a save buffer / a delta buffer that datapath's forward / dgrad wrote
 * A dgrad reads the save buffer of a forward of its own column; bf16x3 and fp16x3 may read each other's (the same tiles), but the
 * weight gradient then refuses the mixed pair.  Any other code is NERF_E_BADARG (the size functions return 0). */

int nerf_abi_version(void);
const char* nerf_last_error(void);

/* ---- parameter vector (replaces nn.Module storage, run_nerf_helpers.py:79-94) ---------- */
int nerf_param_count(void);
/* offset (floats) of tensor #idx of the state_dict (0..23: pts_linears.0.weight, .bias, ...,
 * views_linears.0.*, feature_linear.*, alpha_linear.*, rgb_linear.*); returns -1 if idx is out of range.
 * rows/cols receive the tensor shape (cols = 1 for biases). */
int nerf_param_offset(int idx, int* rows, int* cols);
/* size of the MFMA-fragment repack of one network (floats) */
int nerf_packed_floats(void);
/* canonical parameters -> fragment streams consumed by nerf_field_fwd / nerf_field_bwd.
 * Call after every optimizer step. */
int nerf_pack_params(const float* params, float* packed, void* stream);

/* test hook (host only, no GPU): out_host[i] = index into the canonical vector that packed[i] is gathered
 * from, or -1 for zero padding; nerf_packed_floats() entries. */
int nerf_debug_pack_table(int* out_host);

/* ---- Embedder.embed (run_nerf_helpers.py:15-45): x[n_pts][3] -> out[n_pts][3 + 6*n_freqs] */
int nerf_embed(const float* x, long n_pts, int n_freqs, float* out, void* stream);

/* ---- z_vals of render_rays (run_nerf.py:357-379).  t_vals = torch.linspace(0,1,n_samples);
 * t_rand [n_rays][n_samples] uniform draws or NULL (perturb == 0). */
int nerf_sample_coarse(const float* rays, int ray_stride, int n_rays, const float* t_vals, int n_samples,
                       int lindisp, const float* t_rand, float* z_vals, void* stream);

/* ---- ray set-up of render(c2w=...) (run_nerf.py:95-123): get_rays (run_nerf_helpers.py:153-162), normalised view
 * directions (:100-107; taken from c2w even when c2w_staticcam supplies the rays), ndc_rays(H, W, K[0][0], 1., ...)
 * (helpers:175-192) when ndc != 0, and the near / far columns, written as rays[H*W][ray_stride] records
 * (o3, d3, near, far, viewdir3), pixel (row j, column i) at j*W + i.  K_host: HOST pointer to the 3x3 intrinsics,
 * row-major; c2w_host / c2w_staticcam_host (nullable): HOST pointers to 3x4 row-major poses (they travel as kernel
 * arguments; no device copy).  rays: device. */
int nerf_make_rays(int H, int W, const float* K_host, const float* c2w_host, const float* c2w_staticcam_host, int ndc,
                   float near, float far, float* rays, int ray_stride, void* stream);

/* ---- ray records of render(rays=(rays_o, rays_d), use_viewdirs=True) (run_nerf.py:95-123, no c2w / c2w_staticcam):
 * rays_o / rays_d [n_rays][3] device, fp32, contiguous (world space).  View directions rays_d / |rays_d| (:100-107), then
 * ndc_rays(H, W, focal, 1., ...) (run_nerf_helpers.py:175-192) iff ndc != 0, then the near / far columns (:117-123):
 * rays[n_rays][ray_stride] = (o3, d3, near, far, viewdir3).  focal = K[0][0]; H, W, focal are read only when ndc != 0. */
int nerf_assemble_rays(const float* rays_o, const float* rays_d, long n_rays, int ndc, int H, int W, float focal, float near,
                       float far, float* rays, int ray_stride, void* stream);

/* ---- the ray batch of one train() step in the reference's 'no_batching' mode (run_nerf.py:726-757): n_rand DISTINCT pixels of one
 * image -- of the window (h0, w0, nh, nw): the central crop of the first precrop_iters steps (:738-747), or the whole image --, their
 * rays as get_rays gives them (run_nerf_helpers.py:153-162) and their colours:
 *   batch_rays[2][n_rand][3] = (rays_o, rays_d), target[n_rand][3] = image[j][i], pixels[n_rand] = j * W + i (nullable).
 * The reference builds the [H,W,3] ray grid and a meshgrid and draws np.random.choice(H*W, N_rand, replace=False) on the host every
 * step; here pixel k of the batch is perm(k), a keyed bijection of [0, nh*nw) (6-round Feistel network, cycle-walked): distinct by
 * construction, and WHICH subset is decided by (key0, key1), two words the host draws per step from its own generator -- no O(H*W)
 * work, no device synchronisation.  K_host: HOST 3x3 intrinsics; pose: DEVICE c2w[:3,:4], rows pose_row_stride floats apart (a
 * slice of a [N,4,4] pose table stays where it is); image: DEVICE [H][W][3] fp32. */
int nerf_sample_ray_batch(int H, int W, const float* K_host, const float* pose, int pose_row_stride, const float* image, int h0,
                          int w0, int nh, int nw, int n_rand, unsigned key0, unsigned key1, float* batch_rays, float* target,
                          int* pixels /* nullable */, void* stream);
/* ---- the use_batching mode of train() (run_nerf.py:676-726; additive in ABI v10): batch `batch` of one epoch over the (view, pixel)
 * space of n_views training views.  The reference builds rays_rgb [V*H*W, 3, 3] once on the host, shuffles it and slices consecutive
 * N_rand windows; here position p of the epoch is perm(p), the keyed bijection of nerf_sample_ray_batch applied to [0, V*H*W) and
 * keyed by (key0, key1), one pair per epoch, and the batch is positions [batch*n_rand, min((batch+1)*n_rand, V*H*W)): the last batch of
 * an epoch is short, as the reference's slice is.  Position q = v*H*W + j*W + i is pixel (j, i) of view view_ids[v].  Rays come from
 * the pose table as it is at this launch (no precrop: the reference applies none in this mode).
 *   view_ids: DEVICE int32 [n_views] indices into the tables (i_train); an index outside [0, n_table) reads nothing and yields NaN;
 *   poses: DEVICE c2w, view t at poses + t*pose_view_stride, rows pose_row_stride floats apart ([N,3,4], [N,4,4] or a view of either);
 *   images: DEVICE [H][W][3] fp32 per view, view t at images + t*image_view_stride; K_host: HOST 3x3.
 * Writes B = min(n_rand, V*H*W - batch*n_rand) rays: batch_rays[2][B][3] = (rays_o, rays_d) as get_rays gives them, target[B][3],
 * pixels[B] = j*W + i and views[B] = v (both nullable).  NERF_E_BADARG if V*H*W >= 2^32 or batch*n_rand >= V*H*W. */
int nerf_sample_ray_views(int H, int W, const float* K_host, const int* view_ids, int n_views, int n_table, const float* poses,
                          long pose_view_stride, int pose_row_stride, const float* images, long image_view_stride, int n_rand, long batch,
                          unsigned key0, unsigned key1, float* batch_rays, float* target, int* pixels /* nullable */,
                          int* views /* nullable */, void* stream);
/* Adjoint of the ray set-up of nerf_sample_ray_batch / nerf_sample_ray_views w.r.t. the camera poses: from d_batch_rays[2][n_rays][3]
 * (d rays_o, d rays_d), the pixels (j*W + i) and views (position in the view list; NULL = all rays belong to view 0, n_views = 1) of
 * the same batch, d_pose[n_views][3][4] (accumulate ? += : =) with dR[a][b] = sum_k d_rd[k][a] dir_k[b] and dt[a] = sum_k d_ro[k][a],
 * dir_k recomputed from the pixel with the forward's arithmetic.  Fixed-order sums, no atomics: bit-reproducible; a view without a ray
 * gets exact zeros. */
int nerf_ray_pose_grad(int W, const float* K_host, const float* d_batch_rays, int n_rays, const int* pixels, const int* views /* nullable */,
                       int n_views, float* d_pose, int accumulate, void* stream);

/* ---- network_query_fn(pts, viewdirs, network_fn) with pts = o + d*z
 * (run_nerf.py:381,385 -> run_network :37-51 -> Embedder :44-45 -> NeRF.forward helpers:96-119).
 * raw[n_rays][n_samples][4] = (rgb pre-sigmoid, sigma pre-relu).
 * act: NULL for inference; otherwise nerf_act_floats() floats that receive what the backward needs. */
size_t nerf_act_floats(int n_rays, int n_samples);
/* Scratch of one training call of render_rays (run_nerf.py:308-418) on n_rays rays, in floats: the saved activations of
 * the coarse pass (n_coarse samples) and of the fine pass (n_coarse + n_fine samples; none if n_fine == 0), plus the
 * deltas and the per-chunk partial weight gradients of the larger pass (reused by both backward calls).  The caller
 * owns this memory (persistent across steps; any datapath); 0 when training == 0 -- inference needs no scratch.
 * = nerf_act_floats(coarse) + nerf_act_floats(fine) + nerf_delta_floats(larger) + nerf_wgrad_partial_floats(larger). */
size_t nerf_workspace_floats(int n_rays, int n_coarse, int n_fine, int training);
/* The same three sizes for ONE datapath (ABI v9; `datapath`: the sizes row of the datapath table -- 10.6 KB / point each way on
 * fp32 rows, 4.8 / 4.4 KB on 16-bit tiles, twice that with two-word saves); the two-argument forms above return the larger of 0
 * and 1, i.e. a buffer either of those may write.  A caller that knows its datapath keeps ~2.2x more rays resident per GB of HBM with these:
 * the 32,768-ray batch of BASELINE configs[3] holds ~40 GB of saved activations on the split datapaths instead of ~90 GB. */
size_t nerf_act_floats_dp(int n_rays, int n_samples, int datapath);
size_t nerf_delta_floats_dp(int n_rays, int n_samples, int datapath);
size_t nerf_workspace_floats_dp(int n_rays, int n_coarse, int n_fine, int training, int datapath);
int nerf_field_fwd(const float* packed, const float* rays, int ray_stride, const float* z_vals, int n_rays,
                   int n_samples, float* raw, float* act, void* stream);

/* ---- raw2outputs (run_nerf.py:262-305).  rays_d points at the first direction component of ray 0,
 * consecutive rays are dir_stride floats apart (3 for a bare [N,3] tensor, 11 for rays + 3).
 * noise: standard-normal draws [n_rays][n_samples] or NULL; weights / depth_map may be NULL. */
int nerf_raw2outputs(const float* raw, const float* z_vals, const float* rays_d, int dir_stride, int n_rays,
                     int n_samples, const float* noise, float raw_noise_std, int white_bkgd, float* rgb_map,
                     float* disp_map, float* acc_map, float* weights, float* depth_map, void* stream);
/* autograd of raw2outputs w.r.t. raw (all five outputs of run_nerf.py:305 are differentiable in the reference):
 * d_rgb[n_rays][3] required; d_acc / d_disp / d_depth [n_rays] and d_weights [n_rays][n_samples] may be NULL. */
int nerf_raw2outputs_bwd(const float* raw, const float* z_vals, const float* rays_d, int dir_stride, int n_rays,
                         int n_samples, const float* noise, float raw_noise_std, int white_bkgd,
                         const float* d_rgb, const float* d_acc, const float* d_disp, const float* d_weights,
                         const float* d_depth, float* d_raw, void* stream);

/* ---- distortion loss of the compositing weights (mip-NeRF 360's regulariser; additive in ABI v10; not in the reference).  Per ray
 * with depths z_0 <= ... <= z_{S-1} (the CALLER's contract, not checked), weights w_i and the ray's own near / far:
 *   s_i = (z_i - near) / (far - near), or 0 for every i when far - near is not > 0 (such a ray has loss 0 and gradient 0);
 *   sample i < S-1 owns [s_i, s_{i+1}]: m_i = (s_i + s_{i+1}) / 2, dl_i = s_{i+1} - s_i; the last sample owns a zero-length
 *   interval, m_{S-1} = s_{S-1}, dl_{S-1} = 0 (its compositing distance of 1e10 is a sentinel, not a length);
 *   loss[r] = sum_i sum_j w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 dl_i
 *   dloss/dw_k = 2 sum_j w_j |m_k - m_j| + 2/3 w_k dl_k
 * evaluated in O(n_samples) from exclusive prefix and (directly summed) suffix sums of w and w m, one wavefront per ray, lane
 * segments and wave scans as in nerf_raw2outputs; no atomics: the same inputs give the same bits.  near_far[0], near_far[1] are ray
 * 0's near and far, ray r's lie r * nf_stride floats further on (rays + 6 with stride 11 for ray records; stride 0: one pair for
 * all rays).  No gradient to z_vals, near or far: depths are constants of the graph.  1 <= n_samples <= 4096; n_rays = 0 launches
 * nothing.  Reads 8 B per point, writes 4 B per ray. */
int nerf_distortion_fwd(const float* weights, const float* z_vals, const float* near_far, int nf_stride, int n_rays,
                        int n_samples, float* loss, void* stream);
/* its adjoint, recomputed from the inputs (nothing saved): d_weights[r][k] = d_loss[r] * dloss/dw_k, written (accumulate = 0) or
 * added to what d_weights holds (accumulate = 1).  Reads 8 B per point (12 B with accumulate), writes 4 B per point. */
int nerf_distortion_bwd(const float* weights, const float* z_vals, const float* near_far, int nf_stride, int n_rays,
                        int n_samples, const float* d_loss, float* d_weights, int accumulate, void* stream);

/* ---- interlevel loss of proposal weights against a target histogram (mip-NeRF 360's proposal loss; additive in ABI v10; not in the
 * reference).  Per ray: proposal depths zp_0 <= ... <= zp_{P-1} with weights wp_i, target depths z_0 <= ... <= z_{S-1} with weights w_j
 * (sorted depths are the CALLER's contract, not checked).  Sample k of either side owns the half-open interval from its depth to the
 * next one, the last sample [depth_last, +inf).  Intervals j and i overlap when max(z_j, zp_i) < min(z_{j+1}, zp_{i+1}), +inf behind
 * each last depth: a zero-length interval overlaps nothing, the two last intervals always overlap.
 *   bound_j = sum of wp_i over the proposal intervals overlapping target interval j, added in ascending i in fp32 (a direct sum)
 *   loss[r] = sum_j max(0, w_j - bound_j)^2 / (w_j + 1e-7)
 *   dloss/dwp_i = sum over the j overlapping i, in ascending j, of -2 max(0, w_j - bound_j) / (w_j + 1e-7)
 * One wavefront per ray, the proposal row staged in LDS; every lane finds the contiguous run of candidates of its interval by binary
 * search, applies the predicate to each and sums in order; no atomics: the same inputs give the same bits.  At most P + S - 1 pairs
 * overlap: linear work per ray.  The target side is a constant of the graph: no gradient to w, to either set of depths.
 * 1 <= n_proposal, n_samples <= 4096; n_rays = 0 launches nothing.  Reads 8 B per proposal point and 8 B per target point, writes 4 B
 * per ray. */
int nerf_interlevel_fwd(const float* proposal_weights, const float* proposal_z, int n_proposal, const float* weights,
                        const float* z_vals, int n_samples, int n_rays, float* loss, void* stream);
/* its adjoint, bound_j recomputed from the inputs (nothing saved): d_proposal_weights[r][i] = d_loss[r] * dloss/dwp_i, gathered per
 * proposal interval, written (accumulate = 0) or added to what d_proposal_weights holds (accumulate = 1).  Reads 8 B per proposal
 * point (12 B with accumulate) and 8 B per target point, writes 4 B per proposal point. */
int nerf_interlevel_bwd(const float* proposal_weights, const float* proposal_z, int n_proposal, const float* weights,
                        const float* z_vals, int n_samples, int n_rays, const float* d_loss, float* d_proposal_weights,
                        int accumulate, void* stream);

/* ---- hierarchical sampling (run_nerf.py:392-396,412 + sample_pdf, run_nerf_helpers.py:196-239):
 * z_mid, sample_pdf(z_mid, weights[1:-1], n_fine, det = (u == NULL)), sort(cat(z_vals, z_samples)), z_std.
 * u [n_rays][n_fine] uniform draws or NULL; u_lin = torch.linspace(0,1,n_fine) (read when u == NULL).
 * z_all [n_rays][n_coarse+n_fine]; z_samples [n_rays][n_fine] may be NULL. */
int nerf_sample_fine(const float* z_vals, const float* weights, int n_rays, int n_coarse, int n_fine,
                     const float* u, const float* u_lin, float* z_all, float* z_samples, float* z_std, void* stream);

/* ---- sample_pdf (run_nerf_helpers.py:196-239) in its standalone form: bins[n_rays][n_bins],
 * weights[n_rays][n_bins-1] -> samples[n_rays][n_samples]; det = (u == NULL). */
int nerf_sample_pdf(const float* bins, const float* weights, int n_rays, int n_bins, int n_samples,
                    const float* u, const float* u_lin, float* samples, void* stream);

/* ---- backward of nerf_field_fwd: d_raw[n_rays][n_samples][4] -> gradient of the flat parameter vector
 * (autograd of run_nerf_helpers.py:96-119; parameters only).
 * delta / partial: scratch of nerf_delta_floats() / nerf_wgrad_partial_floats() floats.
 * accumulate != 0 adds into grad, otherwise grad is overwritten. */
size_t nerf_delta_floats(int n_rays, int n_samples);
size_t nerf_wgrad_partial_floats(int n_rays, int n_samples);
int nerf_field_bwd(const float* packed, const float* act, const float* d_raw, int n_rays, int n_samples,
                   float* delta, float* partial, float* grad, int accumulate, void* stream);

/* the two halves of nerf_field_bwd, separately launchable (bench.py brackets each with HIP events):
 * dgrad: d_raw -> per-layer deltas;  wgrad: (deltas, saved activations) -> parameter gradient. */
int nerf_field_dgrad(const float* packed, const float* act, const float* d_raw, int n_rays, int n_samples,
                     float* delta, void* stream);
int nerf_field_wgrad(const float* act, const float* delta, const float* d_raw, int n_rays, int n_samples,
                     float* partial, float* grad, int accumulate, void* stream);

/* ---- the three-term SPLIT datapaths of the same functions (csrc/split_types.h): every product W x of the MLP is evaluated
 * as  W_hi x_hi + W_hi x_lo + W_lo x_hi  on 16-bit MFMAs with fp32 accumulation, hi = T(v), lo = T(v - hi):
 *   split = 1, T = IEEE half ("fp16x3", the host code's default): v_mfma_f32_16x16x32_f16 / 32x32x16_f16, ~2^-22 per product --
 *              fp32-class; the rows / deltas saved for the weight-gradient GEMM are the hi words (11 significant bits);
 *   split = 0, T = bfloat16 ("bf16x3"): ~2^-17 per product, 8-bit saved operands; fp32's exponent range (no overflow possible).
 * Judged by the north-star PSNR criterion (measured: 4e-6 / 2.4e-4 dB) and by fp64 comparisons of the gradients (tests/).
 * Parameters are repacked into (hi, lo) fragment streams of nerf_packed3_floats() 32-bit words by nerf_pack_params_split
 * (streams = mask of 1: 16-point forward stream, 4: transposed streams of the delta chain -- 5 = everything these entry points
 * read).  feature_linear is
 * FOLDED into the view branch: W' = Wv[:, :256] Wf, b' = Wv[:, :256] bf + bv are derived at pack time (helpers:111-115: no activation
 * between the two layers); `feature` and its delta are neither computed nor saved, and the weight-gradient entry point takes the
 * canonical parameter vector `params` (the one that was packed) to produce the gradients of Wf, bf and Wv[:, :256] from
 * G = delta_hv^T h7:  dWv[:, :256] = G Wf^T + dbv bf^T,  dWf = Wv[:, :256]^T G,  dbf = Wv[:, :256]^T dbv.
 *   Kernels: 16 points per wavefront at 2 waves / SIMD, weights through a 17-slot LDS ring of 8 KiB fragment units (csrc/field_ring.h);
 * the delta chain 32 points per wavefront on the same ring.  The save buffers hold 16-bit elements in tiles (rows of the 256- /
 * 128-wide regions in 16-point tiles, row16h order; deltas and encodings in 32-point feature-major tiles; csrc/nerf_common.h), the
 * ReLU bitmask words are in these kernels' lane order: forward, dgrad and weight gradients of one evaluation must use the same split.
 *   Range (split = 1): weights, encodings and activations must stay below 65520 in magnitude (a NeRF's are O(1..100)); an overflow
 * turns into inf / NaN in `raw` (the ReLU propagates NaN).  Deltas are tiny (upstream gradients ~1e-6): nerf_field_dgrad_split(split
 * = 1) first reduces max|d_raw| on the device and runs the chain on s * d_raw with s the power of two that puts that maximum in
 * [16, 32) (the chain is linear; the maximum lives in the delta buffer), every stored delta and partial weight gradient carries s, and
 * the reduction phase of nerf_field_wgrad_phase multiplies by 1/s -- exact.  A non-finite d_raw propagates to the gradient.
 *   split = 5 (ABI v10, "fp16x3w"): the fp16 split with TWO-WORD saves -- the forward and the delta chain store the lo words
 * (T(v - hi)) next to the hi words (mirror regions at ActLayout3::lo / DeltaLayout3::lo), and the weight-gradient GEMM contracts
 * d_hi^T X_hi + d_hi^T X_lo + d_lo^T X_hi : the products of the forward's class (~2^-22) instead of 11-bit operands, at twice the saved
 * bytes and three times the GEMM's MFMAs.  Not the default: it prices and bounds what the one-word operand storage costs the gradients.
 * Replace run_nerf.py:37-51 + run_nerf_helpers.py:15-45, :96-119 and their autograd like nerf_field_fwd / nerf_field_bwd. */
int nerf_packed3_floats(void);
int nerf_pack_params_split(const float* params, float* packed3, int streams, int split, void* stream);
/* the repack of TWO networks (a training step's coarse and fine network after the optimizer step) in the same two launches as one
 * (ABI v9; results identical to two nerf_pack_params_split calls) */
int nerf_pack_params_split_pair(const float* params_a, float* packed3_a, const float* params_b, float* packed3_b, int streams,
                                int split, void* stream);
int nerf_field_fwd_split(const float* packed3, const float* rays, int ray_stride, const float* z_vals, int n_rays,
                         int n_samples, float* raw, float* act /* nullable: inference */, int split, void* stream);
int nerf_field_dgrad_split(const float* packed3, const float* act, const float* d_raw, int n_rays, int n_samples,
                           float* delta, int split, void* stream);
/* Range check of the fp16 split (ABI v10; replaces the reference's DEBUG-gated NaN / Inf check, run_nerf.py:414-416, with a warning
 * that can come BEFORE the NaN).  buf = what a SAVING fp16 forward left in `act` (nerf_field_fwd_split(split = 1 / 5) with act: the
 * post-ReLU rows of the eight trunk layers and of the view branch, i.e. every value that enters a contraction as an fp16 operand), or
 * what an fp16 delta chain left in `delta` (nerf_field_dgrad_split(split = 1 / 5): the scaled deltas of the same layers, by magnitude).
 * Merges into FOUR caller-owned 32-bit device words: rows -> words[1] = max(words[1], largest fp16 bit pattern), words[0] |= 1 when that
 * pattern is >= 0x7800 (32768: half way to the 65520 beyond which `raw` / the gradient turn NaN); deltas -> words[3], words[2] likewise
 * (NaN patterns compare above inf).  One streaming read (4.2 KB per point at HBM rate: 0.6 ms for 786 k points); the hot kernels carry no
 * monitor (a running maximum costs the saving forward the 6 registers it has left: measured, spills).  The host code scans every
 * NERF_RANGE_CHECK_EVERY-th training render (default 64: 0.2 % of the step time) and reads the words without synchronising. */
int nerf_range_scan(const float* buf, int n_rays, int n_samples, unsigned* words, void* stream);
/* test hooks (host only): gather tables of the fragment streams -- out_host[e] for every 16-bit element e: 2 * canonical_index +
 * is_low_part, or -1 for zero padding (nerf_debug_pack3_table: the (hi, lo) streams incl. the transposed ones, declared below;
 * nerf_debug_pack16_table: the 16-point forward stream). */
int nerf_debug_pack16_table(int* out_host);
/* ---- reduced product class for INFERENCE: split = 2 of nerf_pack_params_split / nerf_field_fwd_split (act must be NULL).
 * Every product of the 256-wide contractions (layers 1..7, the trunk part of the view branch) is  W_hi16 x_hi16  on the fp16 MFMA
 * plus the two correction terms  W_hi8 x_lo8 + W_lo8 x_hi8  as block-scaled fp8 e4m3 MFMAs of K = 128 (v_mfma_scale_f32_16x16x128_
 * f8f6f4): ~2^-15 per product at 2 instead of 3 MFMA-equivalents (csrc/field_ring8.h).  Admitted for inference by the north-star
 * gate with >= 30x margin on both fixtures (profiles/r04_accuracy_classes.md), never used for training.  Activations must stay
 * below 224 in magnitude (NaN beyond).  split = 3: the same pass with sample n_samples - 1 of every ray left unwritten.
 *   nerf_field_fwd_last_sample evaluates every ray's LAST sample of a pass with the three-term fp16 products (packed3 = the
 * split = 1 repack of the same parameters) into the pass's raw: the reference's dists[-1] = 1e10 (run_nerf.py:277-278) makes that
 * sample's alpha a step function of the sign of its density (:293), the one place where a 2^-15 error can move a ray's opacity
 * by O(1).  Call it after a split = 2 pass or in any order with a split = 3 pass, before raw2outputs.
 *   packed3_next (nullable): in the same launch, the last sample of the hierarchical pass that refines this one, evaluated by THAT
 * pass's network into raw_next[n_rays][n_samples_next][4].  Its depth is this pass's last depth: sample_pdf draws inside
 * [z_mid[0], z_mid[-1]] (run_nerf.py:392-396, helpers:196-239), so the sorted union of run_nerf.py:396 ends with z_vals[:, -1].
 * (One launch costs one pass of a workgroup through the network, ~70 us, for one network or two.) */
int nerf_field_fwd_last_sample(const float* packed3, const float* rays, int ray_stride, const float* z_vals, int n_rays,
                               int n_samples, float* raw, const float* packed3_next /* nullable */, float* raw_next,
                               int n_samples_next, void* stream);
/* ---- which layout a scratch buffer holds.  The save buffer of a forward and the delta buffer of a dgrad exist in three layouts each
 * (fp32 point-major rows; bf16 tiles; fp16 tiles: csrc/nerf_common.h); the entry point that writes a buffer decides, and the entry
 * points that read it must agree.  The library remembers per buffer ADDRESS what its own entry points last wrote there (host-side
 * table only; nothing is stored on the device and no pointer is dereferenced later) and
 *   - every dgrad / weight-gradient entry point returns NERF_E_BADARG when given a buffer of the wrong family, of another
 *     ray / sample count, or an (act, delta) pair that no datapath contracts -- instead of computing garbage;
 *   - nerf_field_wgrad_phase(datapath = -1) takes the datapath from the record.
 * Buffers the library has not written (copies, foreign producers) are not checked.
 * nerf_buffer_layout: the recorded kind (the act kind / delta kind rows of the datapath table; *is_delta says which), or -1 for an
 * unknown buffer.  Save buffers hold point-major rows (fp32) or 16-point tiles, delta buffers rows or 32-point tiles. */
int nerf_buffer_layout(const float* buf, int* is_delta, int* n_rays, int* n_samples);
/* test hook (host only): where the regions of such a buffer start, in floats from its base, for n_rays x n_samples points.
 * family: the layout row of the datapath table (2 = the offsets of family 1 plus [15] = offset of the mirror that holds the lo
 * words; [14] total = twice family 1's).  out_host[16]:
 *   save buffer  (is_delta = 0): [0..7] post-ReLU rows of trunk layers 0..7, [8] feature (fp32 rows only; the split datapaths fold
 *                that layer and use the slot as the dump tile of out-of-range waves), [9] view branch, [10] xyz encoding,
 *                [11] direction encoding per ray, [12] its per-point / per-ray-record expansion, [13] ReLU bitmasks, [14] total;
 *   delta buffer (is_delta = 1): [0..7], [8], [9] as above, [10] tiled copy of d_raw, [11] the launch's max|d_raw| word
 *                (family 1 only), [14] total.   Unused slots are -1. */
int nerf_debug_layout(int n_rays, int n_samples, int family, int is_delta, long long* out_host);
/* The weight gradients dW = delta^T x, db = sum delta of one evaluation (the second half of nerf_field_bwd; the only form on the
 * split datapaths), split into launches a profiler can bracket: phases bit 0 = the GEMM jobs (fp32: the eight full-width 256x256
 * jobs; split datapaths: all jobs on the streaming 16-bit GEMM), bit 1 = the six narrow jobs (fp32 datapath only), bit 2 =
 * reduction of the per-chunk partial gradients into grad (deterministic, no atomics; + the folded feature layer's gradients).
 * Calling it with phases 1, 2, 4 in that order equals one call with 7. */
int nerf_field_wgrad_phase(const float* act, const float* delta, const float* d_raw, int n_rays, int n_samples,
                           float* partial, float* grad, int accumulate,
                           int datapath /* the wgrad row of the datapath table; -1 as recorded for act / delta (above) */,
                           int phases, const float* params /* canonical parameters; may be NULL for datapath 0 */,
                           void* stream);
/* ---- dead-tile skipping in the backward of the split datapaths (additive entry points; ABI version unchanged).
 * A 32-point tile (points 32 t .. 32 t + 31 of the launch) is DEAD when all 128 words of its d_raw are +-0 (bits & 0x7fffffff == 0;
 * NaN, Inf and subnormals make a tile live).  Compositing gives every sample whose density is not positive an exactly zero d_raw,
 * the delta chain is linear in d_raw, and a zero delta adds +-0 to every weight and bias gradient: as long as the saved activations
 * are finite, leaving the dead tiles out changes no bit of the gradient.  (With an Inf / NaN activation the dense forms produce
 * 0 * Inf = NaN in that gradient and the sparse forms do not; the fp16 range guard has failed long before.)
 *   nerf_live_tiles_words(n_rays, n_samples): 32-bit words of the caller-owned list buffer `live` of one pass (16-byte aligned).
 *   nerf_field_dgrad_split_live: nerf_field_dgrad_split that also writes `live` -- [0] the count of live tiles, [1] the number of
 * tiles, [4 + i] the live tile numbers in ascending order (then a bitmap and its prefix counts: csrc/launchers.h) -- on the device,
 * without a read-back, in the pass over d_raw that finds its maximum plus one small launch, and runs the delta chain over the live
 * tiles only.  CONTRACT: a dead tile's deltas are NOT WRITTEN (the buffer keeps whatever it held); readers other than
 * nerf_field_wgrad_phase_live with the same list (nerf_field_input_grad, nerf_range_scan on the delta buffer) need the dense form.
 *   nerf_field_wgrad_phase_live: nerf_field_wgrad_phase whose GEMM streams the live tiles only (same chunk plan, same order of
 * summation inside every chunk: the same partial sums minus exact zeros).  datapath 0 (fp32) has no sparse form.
 *   The two go together: when n_samples is a multiple of 32, nerf_field_dgrad_split_live (live != NULL) also writes the per-ray direction
 * encoding, replicated for the GEMM, into scratch inside `act`, and nerf_field_wgrad_phase_live (live != NULL) reads it there instead
 * of writing it itself: call it on the `act` of a nerf_field_dgrad_split_live call made since that buffer's forward.
 *   live = NULL in either: exactly the dense entry point.  NERF_BWD_SKIP_DEAD=0 in the environment (read once per process) makes both
 * ignore `live` (nerf_bwd_skip_dead() returns 0 then): the A/B switch. */
size_t nerf_live_tiles_words(int n_rays, int n_samples);
int nerf_bwd_skip_dead(void);
int nerf_field_dgrad_split_live(const float* packed3, const float* act, const float* d_raw, int n_rays, int n_samples,
                                float* delta, int split, unsigned* live /* nullable */, void* stream);
int nerf_field_wgrad_phase_live(const float* act, const float* delta, const float* d_raw, int n_rays, int n_samples,
                                float* partial, float* grad, int accumulate, int datapath, int phases, const float* params,
                                const unsigned* live /* nullable */, void* stream);
/* ---- render_rays in one call (run_nerf.py:308-418 and its autograd): the whole of a ray batch's forward, and the whole of
 * its backward, as ONE entry point each.  They chain the launches above in C -- coarse depths -> field -> raw2outputs
 * [-> sample_pdf + sort -> field -> raw2outputs]; raw2outputs' adjoint -> delta chain -> weight gradients per pass -- in the
 * order the in-repo binding issues them, so the results are bit-identical to it.  What a host provides: the ray records, the
 * random draws in the reference's order (NULL where the reference draws nothing), the packed and canonical parameters, the
 * outputs, and ONE scratch buffer of nerf_render_workspace_floats() floats that lives from the forward to its backward
 * (depths, coarse raw, compositing weights; when training also the saved activations, deltas and partial gradients: ~9.2 KB
 * per sample point on the split datapaths, ~21 KB on fp32 -- split larger ray batches, the reference's `chunk` argument does exactly that).
 *   precision: the NerfRenderCfg row of the datapath table (packed buffers from that column's repack; workspace of
 *   nerf_render_workspace_floats for THIS cfg).
 *   Backward with accumulate = 0: every gradient vector handed in is written -- a network whose pass received no upstream
 *   gradient gets zeros; d_disp / d_acc may be given without d_rgb.
 *   packed_f / params_f / grad_f NULL (or packed_f == packed_c): the fine pass uses the coarse network (network_fine None).
 *   Outputs as the reference's dict: rgb/disp/acc/raw = the last pass (rgb_map, disp_map, acc_map, raw [n, n_coarse + n_fine, 4]);
 *   rgb0/disp0/acc0/z_std = the coarse pass and the std of the fine samples (n_fine > 0 only).
 *   Backward: upstream gradients of the same outputs (any may be NULL; d_raw_out = gradient of `raw`), the forward's `raw`,
 *   noise draws and workspace; the parameter gradients are written (accumulate = 0) or added into grad_c / grad_f. */
typedef struct NerfRenderCfg {
    int n_coarse, n_fine;          /* N_samples, N_importance */
    int lindisp, white_bkgd;
    float raw_noise_std;
    int precision;                 /* the datapath table's NerfRenderCfg.precision row: 0, 1, 3, 5 */
    int reserved;                  /* (round 3: operand storage switch; ignored) */
} NerfRenderCfg;
size_t nerf_render_workspace_floats(const NerfRenderCfg* cfg, int n_rays, int training);
int nerf_render_rays_fwd(const NerfRenderCfg* cfg, const float* packed_c, const float* packed_f, const float* rays, int ray_stride,
                         int n_rays, const float* t_rand, const float* noise_c, const float* u, const float* noise_f,
                         float* rgb, float* disp, float* acc, float* raw, float* rgb0, float* disp0, float* acc0, float* z_std,
                         float* workspace, int training, void* stream);
/* nerf_render_rays_fwd(training = 0) as ONE kernel launch (csrc/render_fused.hip): a workgroup owns 16 rays from the coarse
 * depths (run_nerf.py:357-379) through both networks, raw2outputs (:262-305) and sample_pdf + sort (:392-396) to the final
 * colours.  Same device code as the separate launches: every output is bit-identical to nerf_render_rays_fwd.  Same arguments
 * and workspace (nerf_render_workspace_floats(cfg, n_rays, 0)).  Split datapaths only (precision 1 / 3), and only sample counts
 * for which 16 rays fill whole 128-point tiles in both passes (n_coarse and n_coarse + n_fine multiples of 8, at most 1024
 * samples per ray): nerf_render_infer_supported(cfg) tells; otherwise NERF_E_BADARG. */
int nerf_render_infer_supported(const NerfRenderCfg* cfg);
int nerf_render_rays_infer(const NerfRenderCfg* cfg, const float* packed_c, const float* packed_f, const float* rays, int ray_stride,
                           int n_rays, const float* t_rand, const float* noise_c, const float* u, const float* noise_f,
                           float* rgb, float* disp, float* acc, float* raw, float* rgb0, float* disp0, float* acc0, float* z_std,
                           float* workspace, void* stream);
int nerf_render_rays_bwd(const NerfRenderCfg* cfg, const float* packed_c, const float* packed_f, const float* params_c,
                         const float* params_f, const float* rays, int ray_stride, int n_rays, const float* noise_c,
                         const float* noise_f, const float* raw, const float* d_rgb, const float* d_disp, const float* d_acc,
                         const float* d_raw_out, const float* d_rgb0, const float* d_disp0, const float* d_acc0,
                         float* workspace, float* grad_c, float* grad_f, int accumulate, void* stream);

/* ---- architectures outside the fused kernels (csrc/dense.hip): the reference's layer stack (run_nerf_helpers.py:96-119) for any
 * netdepth / netwidth / skips / multires / multires_views / i_embed = -1 / use_viewdirs = False (run_nerf.py:435-442,
 * helpers:48-50, :93-94, :117), one layer per call.  Row-major matrices with explicit leading dimensions (a layer may read or
 * write a column range of a wider matrix: skip connection, view branch, rgb | alpha -- no concatenations).  The GEMMs are
 * plain library SGEMMs (rocBLAS, exact fp32, atomics off), loaded on first use; the epilogues are HIP kernels.
 *   nerf_build_inputs : x[p] = [enc(o + d z_p) | enc(viewdir)] for every sample point (run_nerf.py:381, :41-47);
 *                       multires / multires_views = number of frequencies, -1 = identity (i_embed = -1);
 *                       rays [N][ray_stride] = (o3, d3, near, far[, viewdir3 in the LAST three columns])
 *   nerf_dense_fwd    : y[P,N] (+)= x[P,K] w[N,K]^T (+ bias) (then ReLU)               = F.linear (+ F.relu), helpers:99-100
 *   nerf_dense_dgrad  : dx[P,K] (+)= dy[P,N] w[N,K]; then dx *= (act > 0) if act       (act = post-ReLU output of the layer below)
 *   nerf_dense_wgrad  : dw[N,K] (+)= dy^T x; dbias[N] (+)= column sums of dy (deterministic two-pass sum; scratch of
 *                       nerf_dense_wgrad_scratch_floats(P, N) floats)
 * The empty batch (P == 0, n_rays == 0) is a valid call and returns 0: the row operands (x, y, dy, dx, act, scratch; rays, z_vals)
 * are not touched and may be NULL, as the data pointer of an empty tensor is; sizes and leading dimensions are still checked, and
 * w / dw must be given.  nerf_dense_wgrad then writes what a sum over no rows is: with accumulate = 0 zeros into dw's N x K range
 * (honouring lddw) and into dbias, on `stream`; with accumulate = 1 nothing. */
int nerf_build_inputs(const float* rays, int ray_stride, const float* z_vals, int n_rays, int n_samples, int multires, int multires_views,
                      int use_viewdirs, float* x, int ldx, void* stream);
int nerf_dense_fwd(const float* x, int ldx, int K, const float* w, int ldw, const float* bias, float* y, int ldy, int N, long P,
                   int accumulate, int relu, void* stream);
int nerf_dense_dgrad(const float* dy, int lddy, int N, const float* w, int ldw, float* dx, int lddx, int K, long P, int accumulate,
                     const float* act, int ldact, void* stream);
size_t nerf_dense_wgrad_scratch_floats(long P, int N);
int nerf_dense_wgrad(const float* dy, int lddy, int N, const float* x, int ldx, int K, long P, float* dw, int lddw, float* dbias,
                     float* scratch, int accumulate, void* stream);

/* ---- img2mse (run_nerf_helpers.py:11: torch.mean((x - y) ** 2), the loss of run_nerf.py:765-772) in one launch, and its
 * gradient w.r.t. x in one more: out[0] = mean((x - y)^2) over n elements (deterministic block-ordered sum); dx = (2 g / n)(x - y)
 * with g = grad_out[0] read on the device.  scratch: nerf_mse_scratch_floats() floats, ZERO before its first use (the kernel
 * leaves it zeroed). */
int nerf_mse_scratch_floats(void);
int nerf_mse_fwd(const float* x, const float* y, long n, float* scratch, float* out, void* stream);
int nerf_mse_bwd(const float* x, const float* y, long n, const float* grad_out, float* dx, void* stream);

/* ---- optimizer.step() of run_nerf.py:776 for torch.optim.Adam(lr, betas=(beta1, beta2), eps) (run_nerf.py:207), fused over
 * a flat vector: params / grads / exp_avg / exp_avg_sq [n]; step = 1-based step count (bias correction). */
int nerf_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int n, float lr, float beta1,
                   float beta2, float eps, int step, void* stream);
/* test hook (host only): out_host[e] for every 16-bit element e of the weight streams (2 * stream words):
 * 2 * canonical_index + is_low_part, or -1 for zero padding. */
int nerf_debug_pack3_table(int* out_host);

/* ---- gradients to the INPUTS of the field and the compositing (additive in ABI v10): rays, sample points, camera poses.
 * The reference differentiates render() end to end (plain autograd); these entry points carry dL/d(ray records). */
/* Input gradient of one field evaluation, enqueued after its dgrad (nerf_field_bwd / nerf_field_dgrad / nerf_field_dgrad_split) and
 * before `delta` is reused: reads the deltas of layers 0 and 5 and of the view branch in whatever layout the dgrad recorded for
 * `delta` (fp32 rows, bf16 / fp16 tiles with the fp16 delta scale, fp16 hi + lo tiles), the fp32 parameter vector `params`
 * (nerf_param_count() floats: W0, W5[:, :63], Wv[:, 256:283] are read), the rays [n_rays][ray_stride] and z_vals
 * [n_rays][n_samples] of the same evaluation, and writes (accumulate = 0) or adds to (accumulate = 1) d_rays[n_rays][11]:
 * columns 0:3 = sum_s dL/dx_s, 3:6 = sum_s z_s dL/dx_s (x_s = o + z_s d), 6:8 = 0 (near / far: no gradient), 8:11 = dL/d viewdir.
 * The sum over a ray's samples has a fixed order (no atomics: bit-reproducible).  n_samples = 1 with z = 0 and d = 0 gives per-point
 * d_pts / d_viewdirs (query_points).  Reads nothing it does not own; changes neither `delta` nor `params`.  NERF_E_BADARG for null
 * pointers, n_samples <= 0, ray_stride < 11, or a `delta` without a matching layout record (unknown buffer, other ray / sample
 * count, a layout without a reader). */
int nerf_field_input_grad(const float* params, const float* delta, const float* rays, int ray_stride, const float* z_vals,
                          int n_rays, int n_samples, float* d_rays, int accumulate, void* stream);
/* nerf_raw2outputs_bwd plus the geometry adjoint: d_rays_d[n_rays][3] = (d / |d|) sum_s dz_s dL/d dist_s (dist_s = dz_s |d|, last
 * dz = 1e10) and d_z_vals[n_rays][n_samples] (through the dists and the depth integral), both WRITTEN; either may be NULL, not both.
 * d_raw is the same as nerf_raw2outputs_bwd's, bit for bit. */
int nerf_raw2outputs_bwd_geom(const float* raw, const float* z_vals, const float* rays_d, int dir_stride, int n_rays,
                              int n_samples, const float* noise, float raw_noise_std, int white_bkgd,
                              const float* d_rgb, const float* d_acc, const float* d_disp, const float* d_weights,
                              const float* d_depth, float* d_raw, float* d_rays_d, float* d_z_vals, void* stream);
/* adjoint of nerf_embed: d_x[n_pts][3] = (accumulate ? d_x + : ) d/dx (out[n_pts][3 + 6 n_freqs] . d_out), the same encoding derivative
 * as nerf_field_input_grad (sin / cos of the exact 2^k x). */
int nerf_embed_bwd(const float* x, long n_pts, int n_freqs, const float* d_out, float* d_x, int accumulate, void* stream);

/* ---- occupancy grid: empty-space skipping for rendering (and, further down, training) (additive in ABI v10; csrc/occupancy.hip).  The reference
 * pushes every sample point of render_rays through the network (run_nerf.py:381-385, :397-401); with a grid only the points in
 * occupied cells are evaluated and every other sample gets raw = (0, 0, 0, 0), i.e. relu(sigma) = 0, alpha = 0, weight 0 (:293).
 *   The grid is an axis-aligned box in the space of the points o + d z the network sees (NDC space for ndc rays), res[0] x res[1] x
 * res[2] cells (1..512 each), one bit per cell: cell (ix, iy, iz) has linear index c = (ix res[1] + iy) res[2] + iz, word c >> 5, bit
 * c & 31 of `bits` (DEVICE, (cells + 31) / 32 words).  Classification of a point p, per axis a: t = (p[a] - lo[a]) * scale[a] -- one
 * fp32 subtraction, one fp32 multiplication, not contracted --, scale[a] = fp32(res[a] / (hi[a] - lo[a])) computed by the host in
 * double; inside iff 0 <= t < res[a] on all three axes (a NaN is outside), cell index floor(t).  A point outside the box counts as
 * occupied (outside_skip == 0: the grid never hides what it does not cover) or as empty (outside_skip != 0). */
typedef struct NerfOccGrid {
    float lo[3];
    float scale[3];
    int res[3];
    int outside_skip;
    const unsigned* bits;
} NerfOccGrid;
/* int32 words of scratch nerf_occ_compact needs for n_points = n_rays * n_samples points (its per-block counts) */
size_t nerf_occ_scratch_words(long n_points);
/* Classify the n_rays * n_samples points o + d z (one fp32 multiply, one fp32 add: run_nerf.py:381) of rays[n_rays][ray_stride] /
 * z_vals[n_rays][n_samples] and compact the occupied ones:
 *   slot[n_rays * n_samples] (int32) = position of the point in the compacted list, or -1;
 *   records[M][11] = (pt3, 0, 0, 0, 0, 0, viewdir3 of the owning ray) in stable ray-major, sample-minor order: n_samples = 1 ray
 *                    records whose depth is 0, evaluated by nerf_field_fwd / nerf_field_fwd_split(n_rays = M, n_samples = 1) with M
 *                    zero depths (o + 0 * 0 == pt exactly); the caller provides room for n_rays * n_samples records;
 *   count[0] = M (one int32 DEVICE word).
 * Three launches -- counts per block of 1024 points, exclusive scan, write -- no atomics: the same inputs give the same list.
 * Moves 8 B per point (z twice) + 4 B (slot) + 44 B per occupied point.  ray_stride >= 11; fewer than 2^31 - 1024 points per call. */
int nerf_occ_compact(const NerfOccGrid* grid, const float* rays, int ray_stride, const float* z_vals, int n_rays, int n_samples,
                     int* slot, float* records, int* count, int* scratch, void* stream);
/* raw[p] = slot[p] >= 0 ? raw_c[slot[p]] : (0, 0, 0, 0) for n_points points of 4 floats (16-byte accesses; raw_c and raw 16-byte
 * aligned; raw_c is not read when no slot is >= 0).  20 B per point + 16 B per occupied point. */
int nerf_occ_expand(const int* slot, const float* raw_c, long n_points, float* raw, void* stream);
/* Grid bits from densities: sigma[n_cells][samples_per_cell] (cell-major) -> bit c of words is set iff any of cell c's values
 * exceeds threshold (a NaN does not); every word of (n_cells + 31) / 32 is written once, whole.  A slice of a grid starting at a cell
 * index that is a multiple of 32 is marked by passing words + first_cell / 32. */
int nerf_occ_mark(const float* sigma, long n_cells, int samples_per_cell, float threshold, unsigned* words, void* stream);
/* bits_out = 3x3x3 OR of bits_in (neighbours beyond the faces do not exist); two different buffers of the grid's size. */
int nerf_occ_dilate(const unsigned* bits_in, int rx, int ry, int rz, unsigned* bits_out, void* stream);
/* ---- training through a grid (additive in ABI v10): the adjoints of the compaction and the density step of occupancy.DensityGrid.
 * d_raw_c[slot[p]] = d_raw[p] for the points with slot[p] >= 0 (4 floats each, 16-byte accesses, both buffers 16-byte aligned): the
 * mirror of nerf_occ_expand.  The slots >= 0 of one nerf_occ_compact call are a bijection onto 0..M-1, so every row < M of d_raw_c
 * [M][4] is written exactly once; d_raw_c must hold M rows.  20 B per point + 16 B per occupied point. */
int nerf_occ_gather(const int* slot, const float* d_raw, long n_points, float* d_raw_c, void* stream);
/* Per-ray gradient of the compacted records' per-point gradient d_rec[M][11] (nerf_field_input_grad on the n_samples = 1 records:
 * columns 0:3 = d/d pt, 8:11 = d/d viewdir).  A record's point is o + d z and its view direction the ray's, so over the samples j of
 * ray r with s = slot[r][j] >= 0:  d_rays[r][0:3] = sum d_rec[s][0:3],  [3:6] = sum z[r][j] * d_rec[s][0:3] (one fp32 product, not
 * contracted),  [6:8] = 0,  [8:11] = sum d_rec[s][8:11] -- nerf_field_input_grad's column contract.  accumulate != 0: added to what
 * d_rays[n_rays][11] holds (columns 6:8 untouched).  One wavefront per ray, lanes stride the samples in ascending order, a butterfly
 * reduction, no atomics: the same inputs give the same bits.  Reads 8 B per point + 24 B per occupied point, writes 44 B per ray. */
int nerf_occ_fold_rays(const int* slot, const float* z_vals, const float* d_rec, int n_rays, int n_samples, float* d_rays, int accumulate,
                       void* stream);
/* density[c] = max(density[c] * decay, max_k sigma[c][k]) for a run of n_cells cells, in place (pass density + first_cell): one fp32
 * multiplication and one maximum; a NaN among the samples counts as -inf; written as m > d ? m : d with d = density[c] * decay. */
int nerf_occ_density_update(const float* sigma, long n_cells, int samples_per_cell, float decay, float* density, void* stream);
/* ---- the occupied span of a ray (additive in ABI v10): per ray (o, d, near, far) = rays[r][0:8] the first and the last occupied
 * stretch it crosses inside [near, far] -- a stretch is one cell, or one stretch outside the box, which counts as occupied iff
 * outside_skip == 0 -- found by two Amanatides-Woo walks over the grid's bits, one from either end:
 *   span[r] = (max(near, t_first - pad), min(far, t_last + pad)),  pad = 2^-10 / max_a |d[a] * scale[a]| (2^-10 cell on the fastest
 *   axis), hit[r] = 1;  or span[r] = (near, far) copied bit for bit and hit[r] = 0 when nothing occupied is crossed, near >= far, a
 *   component of the record is NaN or infinite, or d = 0.
 * Stretches shorter than 2^-10 cell (on the fastest axis) are not looked at: the result lies between the float64 hull of all occupied
 * stretches and that of the stretches longer than 2^-9 cell (OccupancyGrid.ray_span_reference), and on a hit near <= near' < far' <=
 * far.  Both walks take at most res[0] + res[1] + res[2] + 3 steps.  Reads 32 B per ray and the words of the cells walked, writes
 * 12 B per ray; no atomics: the same inputs give the same bits.  ray_stride >= 8; span 8-byte aligned. */
int nerf_occ_ray_span(const NerfOccGrid* grid, const float* rays, int ray_stride, int n_rays, float* span, int* hit, void* stream);
/* ---- importance samples from a density grid (additive in ABI v10): the compositing weights of the samples o + d z (one fp32
 * multiply, one fp32 add) of rays[n_rays][ray_stride] / z_vals[n_rays][n_samples] with the grid's own density as sigma, what
 * render_rays(proposal="grid") hands to nerf_sample_fine in place of a coarse network's weights.  density[cells] (DEVICE) is
 * occupancy.DensityGrid's running maximum per cell.  Lookup of a point, classified as above, no interpolation: inside the box and bit
 * set -> density[c]; inside and bit clear -> 0; outside the box (a NaN included) -> 0 if outside_skip else outside_sigma (the caller
 * passes the grid's sigma_threshold: the least density the grid calls occupied, so the grid still never hides what it does not cover).
 *   weights[r][i] = alpha_i prod_{j<i} (1 - alpha_j + 1e-10),  alpha_i = 1 - expf(-max(sigma_i, 0) * dist_i),
 *   dist_i = (z[i+1] - z[i]) * |d|, the last one 1e10 * |d|  (run_nerf.py:275-293)
 * in the operation order, lane segments and wave scan of nerf_raw2outputs: the weights equal, bit for bit, those nerf_raw2outputs
 * returns for raw = (0, 0, 0, sigma) without noise.  sigma[n_rays][n_samples] (optional, may be NULL) receives the looked-up densities.
 * One wavefront per ray, no colours, no ray integrals, no atomics: the same inputs give the same bits.  Reads 24 B per ray, 4 B per
 * point and one bit word plus one density word per point; writes 4 B (8 B with sigma) per point.  ray_stride >= 6; 1 <= n_samples <= 4096. */
int nerf_occ_proposal_weights(const NerfOccGrid* grid, const float* density, float outside_sigma, const float* rays, int ray_stride,
                              const float* z_vals, int n_rays, int n_samples, float* weights, float* sigma, void* stream);
/* ---- early ray termination for the grid paths (additive in ABI v10): render_rays(early_stop_eps=eps) stops a ray of the refining pass
 * where the COARSE pass's estimate of its transmittance has fallen below eps.  weights[r][i] (nerf_raw2outputs' or
 * nerf_occ_proposal_weights') belongs to the interval [z_i, z_{i+1}] and the sum of the weights up to sample i is 1 - T behind it.
 * Per ray: a = 0; for i = 0 .. n_samples - 1: a = a + weights[r][i] -- one fp32 addition each, strictly left to right (the order is the
 * contract: np.cumsum(weights, axis=1, dtype=float32) is a bit-exact reference) --; i* = the first i with a >= threshold (a NaN never
 * satisfies the comparison and poisons a: such a ray never stops);
 *   z_stop[r] = z_vals[r][i* + 1] if there is an i* and i* + 1 < n_samples, else +inf
 * (the last interval is the reference's 1e10 one: nothing lies behind it).  threshold = fp32(1 - eps), computed by the host in double.
 * The stop is an approximation: what is dropped from the refined image is the REFINING pass's transmittance at z_stop, which is close to
 * eps but not bounded by it.  Weights staged through LDS in tiles of 64 rays x 64 samples (coalesced reads, one lane sums one ray); a
 * block leaves once all of its rays have crossed.  Reads at most 4 B per point (weights) and one z per ray, writes 4 B per ray; no
 * atomics: the same inputs give the same bits.  1 <= n_samples <= 4096. */
int nerf_occ_stop_depth(const float* z_vals, const float* weights, int n_rays, int n_samples, float threshold, float* z_stop, void* stream);
/* nerf_occ_compact with a stop depth per ray (z_stop[n_rays], DEVICE): a point is kept iff it is occupied by nerf_occ_compact's rule AND
 * !(z >= z_stop[ray]) -- a NaN z_stop or a NaN z stops nothing, +inf stops nothing, -inf stops everything.  The comparison comes before
 * the grid lookup: a stopped point reads no bit word.  slot, records, count, scratch, the three launches and the ordering are those of
 * nerf_occ_compact (the same kernels, instantiated with the extra predicate); with z_stop all +inf the results are bit-identical to
 * it.  Moves what nerf_occ_compact moves + 8 B per point (z_stop of the owning ray, twice; cached: 4 B per ray reach HBM). */
int nerf_occ_compact_stop(const NerfOccGrid* grid, const float* rays, int ray_stride, const float* z_vals, const float* z_stop, int n_rays,
                          int n_samples, int* slot, float* records, int* count, int* scratch, void* stream);
/* ---- grid ray marching (additive in ABI v10): render_rays(proposal="march") places the depths of a ray itself instead of thinning
 * out the reference's -- n_steps = M equal steps over [near, far], of which only the ones in occupied cells (and one closing step behind
 * every occupied run) are emitted into n_slots = S slots.  OccupancyGrid.march_reference is the definition.  Per ray (o, d, near, far) =
 * rays[r][0:8], with u[r] in [0, 1) (u == NULL: 0.5 for every ray), for k = 0 .. M - 1:
 *   t_k = (fp32(k) + u) / fp32(M)              one fp32 addition, one correctly rounded fp32 division
 *   z_k = near * (1 - t_k) + far * t_k         run_nerf.py:360's expression: one subtraction, two multiplications, one addition
 *   keep_k  = the point o + d * z_k (one multiply, one add per axis) is occupied by nerf_occ_compact's rule
 *   close_k = !keep_k && k > 0 && keep_{k-1}   the first empty candidate behind an occupied run: it is skipped by the compaction
 *                                              (raw = 0) and owns the gap, so an evaluated sample's interval never reaches across one
 * The emitted candidates are those with keep_k || close_k, in order of k, E of them.  The first n = min(E, S - 1) fill
 * z_vals[r][0 .. n); E > S - 1: truncated[r] = 1 and z_stop[r] = the depth of emitted candidate S - 1 (the first that did not fit);
 * else truncated[r] = 0 and z_stop[r] = far.  z_vals[r][n .. S) = z_stop[r]: nerf_occ_compact_stop's !(z >= z_stop) drops the padding,
 * the last slot (the reference's 1e10 interval) included.  Rows are nondecreasing.  A ray whose first eight components are not all
 * finite, or with near >= far, emits nothing: z_vals[r][:] = its own far (copied bit for bit), z_stop[r] = -inf, truncated[r] = 0.
 * One wavefront per ray, 64 candidates per round (ballots and lane ranks); a wave leaves its loop once S slots are spoken for, so the
 * cost follows what is emitted.  Plain stores, no atomics: the same inputs give the same bits.  Reads 32 B (+ 4 B of u) per ray and
 * one bit word per candidate looked at; writes 4 S + 8 B per ray.  ray_stride >= 8; 1 <= n_steps <= 16384; 1 <= n_slots <= 4096. */
int nerf_occ_march(const NerfOccGrid* grid, const float* rays, int ray_stride, const float* u /* nullable: 0.5 */,
                   int n_rays, int n_steps, int n_slots, float* z_vals, float* z_stop, int* truncated, void* stream);
/* ---- the march with a stop on the grid's own transmittance (additive in ABI v10): render_rays(proposal="march", march_stop_eps=eps).
 * nerf_occ_march over a DensityGrid (density[cells], outside_sigma: nerf_occ_proposal_weights' arguments) with one more rule;
 * DensityGrid.march_stop_reference is the definition.  Candidates, t_k, z_k, keep_k and close_k are nerf_occ_march's.  Per candidate
 *   sigma_k = nerf_occ_proposal_weights' lookup at the point o + d * z_k, taken as 0 unless sigma_k > 0 (a NaN counts as 0)
 *   c_k     = sigma_k * ((z_{k+1} - z_k) * |d|) where keep_k, exactly 0 elsewhere; z_{k+1} is built from fp32(k + 1) by z_k's
 *             expression, and is far for k = M - 1; |d| = sqrt(dx dx + dy dy + dz dz) added left to right; no contraction
 *   A_k     = the exclusive prefix sum of c in fp32 in THIS order: rounds of 64 candidates; inside a round the inclusive scan with
 *             strides 1, 2, 4, 8, 16, 32 (lane l >= stride adds the previous step's value of lane l - stride); A_k = base + incl_{l-1}
 *             (+ 0 for lane 0); base starts at 0 and grows by incl_63 after every round
 *   k_stop  = the first k < M with A_k >= tau (a NaN never satisfies this: a poisoned sum never stops); tau = fp32(-ln(eps)), computed
 *             by the host in double
 * The emitted candidates are those with (keep_k || close_k) && k < k_stop, E of them.  E > S - 1: truncated as by nerf_occ_march,
 * stopped[r] = 0 (the slot limit bit first).  Else, with a k_stop: z_stop[r] = z_{k_stop}, stopped[r] = 1, z_vals[r][E .. S) = z_stop[r].
 * Else everything is nerf_occ_march's, stopped[r] = 0.  Invalid rays: as nerf_occ_march, stopped[r] = 0.  With density all zero the
 * first three outputs are nerf_occ_march's bit for bit.  c >= 0 grows only at kept candidates, so candidate k_stop - 1 is a kept one
 * and its interval ends exactly at z_stop.  AN APPROXIMATION of the render: what is dropped is the network's own transmittance behind
 * z_stop; the grid's densities are a decayed running maximum and overestimate, so that is close to eps where grid and network agree but
 * not bounded by it.  One wavefront per ray, 64 candidates per round (one scan, one more ballot); the wave leaves once the slots are
 * full or the cut has been seen.  Plain stores, no atomics, no LDS: the same inputs give the same bits.  Reads what nerf_occ_march
 * reads and one density word per kept candidate; writes 4 S + 12 B per ray.  ray_stride >= 8; 1 <= n_steps <= 16384;
 * 1 <= n_slots <= 4096; tau > 0. */
int nerf_occ_march_stop(const NerfOccGrid* grid, const float* density, float outside_sigma, const float* rays, int ray_stride,
                        const float* u /* nullable: 0.5 */, int n_rays, int n_steps, int n_slots, float tau, float* z_vals,
                        float* z_stop, int* truncated, int* stopped, void* stream);
/* ---- the march in world-space steps with a per-ray fit to the slots (additive in ABI v10):
 * render_rays(proposal="march", march_step_size=ds, march_fit=J).  OccupancyGrid.march_step_reference (density == NULL) and
 * DensityGrid.march_step_stop_reference (density != NULL) are the definition.  Per ray: |d| = sqrt(dx dx + dy dy + dz dz) added left to
 * right, dz0 = step_size / |d| (one correctly rounded division).  A ray is invalid when its first eight components are not all finite,
 * when near >= far, or when dz0 is not a finite number > 0 (d = 0): z_vals[r][:] = its own far, z_stop[r] = -inf, no flag, level[r] = 0.
 * Level j = 0 .. fit walks with dz_j = dz0 * 2^j, for k = 0 .. n_steps - 1 (n_steps = M is the cap on candidates):
 *   z_k     = near + (fp32(k) + u) * dz_j      one addition, one multiplication, one addition; not contracted; u == NULL: 0.5
 *   valid_k = z_k < far                        z_k is nondecreasing in k: the valid candidates are a prefix
 *   keep_k  = valid_k && the point o + d * z_k is occupied by nerf_occ_compact's rule
 *   close_k = valid_k && !keep_k && k > 0 && keep_{k-1}
 * and from there on everything is nerf_occ_march's with "k < M" read as valid_k: emission in order of k, the first min(E, S - 1) fill
 * the row, E > S - 1 truncates with z_stop = the first candidate that did not fit, else z_stop = far, the padding holds z_stop.
 * With a density, level j also applies nerf_occ_march_stop's rule: c_k = max(sigma_k, 0) * ((z_{k+1} - z_k) * |d|) at kept candidates,
 * z_{k+1} = far where candidate k + 1 is not valid (or k + 1 == M); the same fixed-order prefix sum; k_stop = the first VALID k with
 * A_k >= tau; emission is cut at k_stop; the slot limit bites first.
 * level[r] = the smallest j at which the ray is not truncated, and the outputs are that level's; if no level fits, level[r] = fit and
 * the ray is truncated with that level's outputs.  u is the same at every level.
 * One wavefront per ray, rounds of 64 candidates; a ray that overflows at level j < fit starts again at j + 1 and the plain stores of the
 * later level overwrite its row.  A wave leaves a level once its slots are full, its candidates run out or it stops.  Plain stores, no
 * atomics: the same inputs give the same bits.  stopped must be non-NULL exactly when density is.  ray_stride >= 8;
 * 1 <= n_steps <= 16384; 1 <= n_slots <= 4096; 0 <= fit <= 8; step_size finite and > 0; with a density tau > 0. */
int nerf_occ_march_step(const NerfOccGrid* grid, const float* density /* nullable */, float outside_sigma, const float* rays, int ray_stride,
                        const float* u /* nullable: 0.5 */, int n_rays, float step_size, int n_steps, int n_slots, int fit, float tau,
                        float* z_vals, float* z_stop, int* truncated, int* level, int* stopped /* non-NULL iff density */, void* stream);
/* ---- grids from cameras and silhouettes (additive in ABI v10): project the cells of a grid into n_views training cameras.  World
 * space only (a grid for ndc rays lives in NDC space and is not supported).  OccupancyGrid.view_counts_reference / carved_reference are
 * the definition.  grid gives lo and res (scale and bits are not read); width[a] = fp32((hi[a] - lo[a]) / res[a]) computed by the host
 * in double.  cams[v] = 16 floats: c2w[3][4] row-major (columns right, up, back, position: the reference's get_rays convention), fx,
 * fy, cx, cy.  Corner o in {0,1}^3 of cell (ix, iy, iz): p[a] = lo[a] + fp32(i[a] + o[a]) * width[a] (one multiplication, one addition).
 * In camera v, with d = p - position:  x = d . right,  y = d . up,  s = -(d . back)  -- three products added left to right, not
 * contracted; s is the depth render() samples.  Six inside-tests per corner:
 *   s >= near_m,  s <= far_m,  fx x >= (-m - cx) s,  fx x <= ((W - 1 + m) - cx) s,  -(fy y) >= (-m - cy) s,  -(fy y) <= ((H - 1 + m) - cy) s
 * (m = margin_px; near_m = fp32(near (1 - 2^-10)), far_m = fp32(far (1 + 2^-10)) from the host).  The cell is UNSEEN by v iff all eight
 * corners fail one and the same test (the conservative box-against-frustum test: each test is a half-space); a NaN fails every test.
 *   seen[c] (int32, n_cells) = the number of cameras that see cell c   (accumulate != 0: added to what seen holds)
 * With sat (int32 [n_views][H + 1][W + 1], the summed-area tables of the foreground masks: sat[v][j][i] = foreground pixels with row < j
 * and column < i) camera v CARVES the cell iff all eight corners have s >= near_m, every i = fx x / s + cx and j = cy - fy y / s (IEEE
 * division) is finite, the rectangle i0 = floor(min i - m) .. i1 = ceil(max i + m), j0 .. j1 likewise, lies inside [0, W - 1] x
 * [0, H - 1] (else the camera abstains) and sat[j1+1][i1+1] - sat[j0][i1+1] - sat[j1+1][i0] + sat[j0][i0] == 0: no foreground pixel in
 * it.  The rectangle covers the projection of the whole cell, so no foreground pixel's ray of v crosses a cell that v carves.
 *   carved_words ((n_cells + 31) / 32 words, the grid's bit layout) = the OR over the cameras   (accumulate != 0: ORed into the words)
 * sat and carved_words are both given or both NULL.  One thread per cell, a wave-uniform loop over the views, the four table words
 * loaded only where the camera does not abstain; seen by plain stores, carved_words whole words from a wave ballot (the unused bits of
 * the last word are 0); no atomics: the same inputs give the same bits.  Reads 64 B per view (shared by all cells) and up to 16 B of sat
 * per cell and view; writes 4 B + 1 bit per cell.  n_views >= 1; 1 <= H, W <= 16384; margin_px finite and >= 0. */
int nerf_occ_view_carve(const NerfOccGrid* grid, const float width[3], const float* cams /* [n_views][16] */, int n_views, int H, int W,
                        float near_m, float far_m, float margin_px, const int* sat /* nullable */, int accumulate, int* seen,
                        unsigned* carved_words /* non-NULL iff sat */, void* stream);

/* ---- isosurface (additive in ABI v10): the triangle mesh of a volume at `level`, marching tetrahedra on the Kuhn subdivision of the
 * lattice.  mesh.extract_mesh_reference is the definition, nerf-pytorch_amd/csrc/iso_tables.h holds the tables.  volume is fp32
 * [nx][ny][nz], one value per lattice node; node = (i ny + j) nz + k sits at lo[a] + fp32(index[a]) * step[a].  A node is inside iff
 * value >= level (a NaN is outside).  Every cube (i, j, k), i < nx - 1 ..., is cut into six tetrahedra, one per permutation of the
 * axes.  keep_words (nullable: every cube) holds one bit per cube in the layout of an occupancy grid of resolution (nx - 1, ny - 1,
 * nz - 1); a cube whose bit is 0 emits nothing.
 *   vertices  one per lattice edge with exactly one endpoint inside that belongs to a kept cube, in ascending edge id = 7 node(lower
 *             endpoint) + class (the seven directions 100 010 001 110 101 011 111).  With a, b the values at the lower and upper
 *             endpoint made finite (NaN -> -FLT_MAX, +-inf -> +-FLT_MAX): t = (level - a) / (b - a) (IEEE division; a NaN t is 1/2) and
 *             p = p_a + t (p_b - p_a) per component, nothing contracted.
 *   faces     int32 vertex indices, one triangle per tetrahedron with 1 or 3 inside corners, two with 2, ordered by cube, tetrahedron,
 *             triangle; (p1 - p0) x (p2 - p0) points from inside to outside.
 * The count call fills counts (device int[2]) = (V, F) and the block offsets inside scratch; the emit call, given the same volume,
 * sizes, level, keep_words and scratch afterwards, writes vertices [V][3] and faces [F][3] (and needs V > 0).  Six launches in all: a
 * count per block, a scan and a write for the edges and again for the cubes; plain loads and stores, no atomics: the same inputs give
 * the same bytes.  scratch: as many ints as the size call says (7 per node for the rank of every edge, one per block of 1024 edges and
 * of 256 cubes).  2 <= nx, ny, nz; 7 nodes < 2^31 and 12 cubes < 2^31 (vertex and triangle counts are 32-bit; the size call gives 0
 * otherwise); level finite. */
size_t nerf_iso_scratch_words(int nx, int ny, int nz);
int nerf_iso_count(const float* volume, int nx, int ny, int nz, float level, const unsigned* keep_words /* nullable */, int* scratch,
                   int* counts /* device int[2]: V, F */, void* stream);
int nerf_iso_emit(const float* volume, int nx, int ny, int nz, float level, const float lo[3], const float step[3],
                  const unsigned* keep_words /* nullable */, int* scratch, float* vertices, int* faces, void* stream);

/* ---- baked field (additive in ABI v10): render rays from values stored on the lattice nodes of an occupancy grid, without a network.
 * BakedField.render_rays_reference (nerf-pytorch_amd/baked.py) is the definition.  The grid of resolution (Rx, Ry, Rz) has
 * (Rx + 1)(Ry + 1)(Rz + 1) nodes, node = (i (Ry + 1) + j) (Rz + 1) + k; node_index[node] is the node's row in table, or 0; table is fp16
 * [n_rows][W], row 0 all zeros (it serves every node that is not stored), W = 4 / 16 / 32 halves for sh_degree 0 / 1 / 2.  With
 * B = (sh_degree + 1)^2 a row is sigma, R_0 .. R_{B-1}, G_0 .., B_0 .., zero-padded: the density after the ReLU and the coefficients of
 * the colour LOGITS in the real spherical harmonics Y_0 .. Y_8 of PlenOctrees' order and signs (baked.sh_basis).  Every corner of an
 * occupied cell must have a row; an index outside [0, n_rows) reads row 0.
 * Per ray (11 columns: o, d, near, far, viewdir): the walk of nerf_occ_march_step at level 0 -- |d| added left to right, dz = step_size /
 * |d|; invalid when one of the first eight components is not finite, when near >= far or when dz is not a finite number > 0;
 * z_k = near + (fp32(k) + u) * dz for k = 0 .. max_steps - 1, valid_k = z_k < far, p = o + d * z_k, t = (p - lo) * scale -- and
 *   keep_k = valid_k && 0 <= t < R on all axes && the bit of cell floor(t) is set        (grid->outside_skip is not read: a point
 *                                                                                          outside the box is never sampled)
 * At a kept candidate f = t - floor(t); the eight corner rows are blended in fp32 with the weights (wx wy) wz, w = f or 1 - f, in the
 * order 000 001 .. 111 (x the slowest bit); sigma = max(blend, 0); logit_c = sum_b coefficient_{c,b} * Y_b(viewdir) added left to right
 * (viewdir = columns 8:11, used as given); rgb = 1 / (1 + expf(-logit)); alpha = 1 - expf(-sigma * step_size); the transmittance in
 * front of the candidate is the product of 1 - alpha_j + 1e-10 over the kept j < k (a wave scan inside a round of 64 candidates times
 * the value carried from the rounds before); w = alpha T.
 *   rgb_map [n][3] = sum w rgb (+ 1 - acc with white_bkgd),  acc_map [n] = sum w,  depth_map [n] = sum w z_k,
 *   disp_map [n] = 1 / max(1e-10, depth / acc) with the NaN of 0 / 0 kept (nerf_raw2outputs' expression),
 *   n_samples [n] = the number of kept candidates that were composited; bit 30 (0x40000000) is set on top when a round ended with the
 *                   transmittance below stop_eps (never with stop_eps = 0).
 * stop_eps > 0: behind the first round of 64 candidates at whose end T < stop_eps no further round is walked; what is dropped weighs
 * at most T.  An invalid ray and a ray that keeps nothing give the background, acc = depth = 0 and n_samples = 0.
 * One wavefront per ray; plain loads and stores, no atomics, no LDS: the same inputs give the same bits.  Per kept candidate 32 B of
 * indices and 8 rows of 2 W bytes are read; per ray 28 B are written.  table must be 16-byte aligned.  ray_stride >= 11; sh_degree 0, 1
 * or 2; step_size finite and > 0; 1 <= max_steps <= 2^24; 0 <= stop_eps < 1; n_rows >= 1; n_rays == 0 is a no-op. */
int nerf_baked_render(const NerfOccGrid* grid, const int* node_index, const void* table /* fp16 rows */, int n_rows, int sh_degree,
                      const float* rays, int ray_stride, const float* u /* nullable: 0.5 */, int n_rays, float step_size, int max_steps,
                      float stop_eps, int white_bkgd, float* rgb_map, float* disp_map, float* acc_map, float* depth_map,
                      int* n_samples, void* stream);

/* ---- baked field, training (additive in ABI v10): the render above with stop_eps = 0 and its backward to the table's rows
 * (baked.BakedTrainer; BakedTrainer.render_rays_reference is the definition, DESIGN.md 3.23 the closed form).  No atomics anywhere:
 * every contribution is stored once and summed per destination in a fixed order, so the same inputs give the same bits.
 *   nerf_baked_count: counts [n] = the kept candidates of every ray -- nerf_baked_render's walk without the table, never a stop.
 *   nerf_baked_train_fwd: rgb_map, acc_map, depth_map as nerf_baked_render writes them with stop_eps = 0, bit for bit, and one record
 *     per kept sample at offsets[ray] + (its rank among the ray's kept samples): ray-major, sample-minor.  offsets int [n + 1] is the
 *     exclusive running sum of nerf_baked_count's counts, offsets[n] = total <= 2^30; records [total][12] words, 16-byte aligned:
 *       cell = (ix Ry + iy) Rz + iz and ray (int32), fx, fy, fz, z, e = expf(-sigma step_size), T, c_R, c_G, c_B, gate (1 where the
 *       blended v0 >= 0, else 0).
 *     A position outside [0, total) is not written.
 *   nerf_baked_train_bwd_samples: sample_grads [total][4] = (dL/dv0, dL/dl_R, dL/dl_G, dL/dl_B) of every sample from the upstream
 *     g_rgb [n][3], g_acc [n], g_depth [n]: with alpha = 1 - e, t = 1 - alpha + 1e-10, w = alpha T, g_acc' = g_acc - (G_R + G_G + G_B)
 *     under white_bkgd, q = G . c + g_acc' + g_depth z and S_k = sum_{j > k} q_j w_j (summed back to front, a suffix, never a total
 *     minus a prefix): dL/dalpha = q T - S / t, dL/dv0 = gate dL/dalpha step_size e, dL/dl_c = w G_c c (1 - c).
 *   nerf_baked_train_bwd_rows: grad fp32 [n_rows][W] (W as above), every element written: row_node [n_rows] is the lattice node of a
 *     row (the inverse of node_index; -1 for row 0); order [total] holds the samples sorted by cell, stable (so ascending (ray, k)
 *     inside a cell), cell_start [Rx Ry Rz + 1] the first entry of every cell.  A row's columns are summed over its adjacent cells in
 *     corner order 000 001 .. 111 and each cell's samples in the order of `order`: term = ((wx wy) wz) * contribution, contribution =
 *     dL/dv0 for column 0 and dL/dl_c * Y_b(viewdir of the sample's ray) for column 1 + c B + b, one product and one addition per
 *     term, in three levels of that same order: the consecutive samples of one ray in a cell are summed, these runs are added to
 *     the cell's sum, the cells' sums to the row's.  Row 0, rows without a node and the padding columns are zero.  total == 0 or
 *     n_rays == 0 writes zeros.
 * ray_stride >= 11; sh_degree 0, 1 or 2; step_size finite and > 0; 1 <= max_steps <= 2^24; 1 <= n_rows (<= 2^26 in bwd_rows);
 * 0 <= total <= 2^30; table, records and sample_grads 16-byte aligned.  n_rays == 0 is a no-op in the first three (in bwd_rows rays may
 * then be null).
 *   nerf_baked_train_bwd_rays (csrc/baked_rays.hip; additive in ABI v10): d_rays fp32 [n_rays][11], every element written: the gradient
 *     of the same render with respect to the ray records -- columns 0:3 (o), 3:6 (d) and 8:11 (viewdir); columns 6 and 7 (near, far) are
 *     zeros.  BakedTrainer.render_rays_reference(ray_grad=True) is the definition: the depths z_k, the validity, the
 *     kept set and every sample's cell are constants; f = (o + d z - lo) scale - cell and Y = sh_basis(viewdir) are differentiated, the
 *     normalisation of viewdir is the caller's.  Per record, with a_0 = dL/dv0 (gated) and g_c = dL/dl_c from sample_grads, over the
 *     eight corner rows of the fp16 table in corner order 000 001 .. 111:
 *       m_q[b] = (g_R row_q[1 + b] + g_G row_q[1 + B + b]) + g_B row_q[1 + 2B + b],   r_q = a_0 row_q[0] + sum_b m_q[b] Y_b   (ascending b)
 *       dL/df_x = sum_q (q_x ? + : -) (w_y w_z)_q r_q (likewise y, z),   dL/dY_b = sum_q ((w_x w_y) w_z)_q m_q[b]           (ascending q)
 *       dL/dx = scale * dL/df;   d_o += dL/dx,   d_d += z dL/dx,   d_viewdir += (dY/dviewdir)^T dL/dY.
 *     One wavefront per ray, lane = record, rounds of 64 over offsets[ray] .. offsets[ray + 1].  Order of summation: lane l adds the
 *     records l, l + 64, l + 128, .. of its ray into nine accumulators (d_o, d_d, d_viewdir) in that order, then one xor butterfly over
 *     the lanes, partners at distance 32, 16, 8, 4, 2, 1 in turn, finishes each sum: the same inputs give the same bits.  No atomics, no
 *     LDS, no scratch.  Per record 32 B of the record, 16 B of sample_grads, 32 B of node_index and 8 rows of 2 W bytes are read (what
 *     nerf_baked_train_fwd gathers, plus 16 B); per ray 8 B of offsets and 12 B of viewdir are read and 44 B written.  offsets, a
 *     record's cell and a node's row are checked against their buffers (a record with a cell outside the grid adds nothing, a row
 *     outside the table reads row 0).  Rays without records -- misses, invalid rays -- give zeros.  ray_stride >= 11; sh_degree 0, 1 or
 *     2; n_rows >= 1; 0 <= total <= 2^30; table, records and sample_grads 16-byte aligned.  n_rays == 0 is a no-op; total == 0 writes
 *     zeros. */
int nerf_baked_count(const NerfOccGrid* grid, const float* rays, int ray_stride, const float* u /* nullable: 0.5 */, int n_rays,
                     float step_size, int max_steps, int* counts, void* stream);
int nerf_baked_train_fwd(const NerfOccGrid* grid, const int* node_index, const void* table /* fp16 rows */, int n_rows, int sh_degree,
                         const float* rays, int ray_stride, const float* u /* nullable: 0.5 */, int n_rays, float step_size, int max_steps,
                         int white_bkgd, const int* offsets, int total, float* records, float* rgb_map, float* acc_map, float* depth_map,
                         void* stream);
int nerf_baked_train_bwd_samples(const float* records, const int* offsets, int n_rays, int total, float step_size, int white_bkgd,
                                 const float* g_rgb, const float* g_acc, const float* g_depth, float* sample_grads, void* stream);
int nerf_baked_train_bwd_rows(const NerfOccGrid* grid, const int* row_node, int n_rows, int sh_degree, const float* rays, int ray_stride,
                              int n_rays, const float* records, const float* sample_grads, const int* order, const int* cell_start,
                              int total, float* grad, void* stream);
int nerf_baked_train_bwd_rays(const NerfOccGrid* grid, const int* node_index, const void* table /* fp16 rows */, int n_rows, int sh_degree,
                              const float* rays, int ray_stride, int n_rays, const float* records, const float* sample_grads,
                              const int* offsets, int total, float* d_rays /* [n_rays][11], every element written */, void* stream);

/* ---- baked field, regularisers (additive in ABI v10): total variation and Cauchy sparsity of the fp32 master table over the stored
 * lattice nodes (baked.BakedTrainer.regularizers; baked.regularizer_reference is the definition).  values is fp32
 * [n_rows][W] (W = 4 / 16 / 32 floats for sh_degree 0 / 1 / 2, 16-byte aligned), column 0 the density before the ReLU, columns 1 .. 3B
 * the colour coefficients, the rest padding; node_index and row_node as above.  With n + e_a the next node along axis a,
 *   D_a[n][c] = s_a (v[n + e_a][c] - v[n][c])  where n + e_a lies in the lattice and is stored, else 0     (a missing neighbour is
 *                                                                                                 left out, not taken as zero)
 *   t[n][c]   = sqrtf(((D_x^2 + D_y^2) + D_z^2) + eps)
 * and s_a = (sx, sy, sz) = min(cell edge) / (cell edge along a).
 *   nerf_baked_reg_fwd: terms [n_rows][3], every element written: per stored row (t[n][0], the sum of t[n][c] over c = 1 .. 3B,
 *     log1pf(2 max(v[n][0], 0)^2)); zeros for row 0 and rows without a node.  The colour sum is a butterfly over the row's W lanes,
 *     partners at distance 1, 2, 4, .. W/2 in turn.  The caller sums the rows.
 *   nerf_baked_reg_bwd: grad [n_rows][W], every element written: the gradient of g[0] sum_n t[n][0] + g[1] sum_n sum_c t[n][c] + g[2]
 *     sum_n log1p(..) (g: three floats on the device), gathered per stored row and column -- no atomics --
 *       w_c ( - sum_a s_a D_a[n][c] / t[n][c]  +  sum_a [m = n - e_a stored] s_a D_a[m][c] / t[m][c] )  +  (c == 0) g[2] 4 sg / (1 + 2 sg^2),
 *     w_0 = g[0], w_c = g[1], sg = max(v[n][0], 0): at most 13 rows read per row (n; n + e_a; n - e_a and its two other forward
 *     neighbours), in that written order, the six terms added in that order (own x, y, z, then behind x, y, z).  Row 0, rows without
 *     a node and the padding columns are zero.  The same inputs give the same bits.
 * sh_degree 0, 1 or 2; 1 <= n_rows <= 2^26 (n_rows == 1: all zeros); eps and the three scales finite and > 0; values and grad 16-byte
 * aligned.  An index read from memory that does not address its buffer counts as "not stored". */
int nerf_baked_reg_fwd(const NerfOccGrid* grid, const int* node_index, const int* row_node, const float* values, int n_rows, int sh_degree,
                       float sx, float sy, float sz, float eps, float* terms, void* stream);
int nerf_baked_reg_bwd(const NerfOccGrid* grid, const int* node_index, const int* row_node, const float* values, int n_rows, int sh_degree,
                       float sx, float sy, float sz, float eps, const float* g /* device, 3 floats */, float* grad, void* stream);

/* ---- hash-grid encoding (additive in ABI v10; csrc/hash_encode.hip; hashgrid.HashEncoding): a multiresolution
 * lattice over the box [lo, lo + 1 / inv_extent], level l with (R_l + 1)^3 nodes (corners aligned), every level's rows in ONE fp32
 * table embeddings [rows_total][n_features].  The HOST computes the level tables (Python float64 and integers) and hands them down
 * in this record; the library checks them against each other (level_dense[l] iff (R_l + 1)^3 <= T = 2^log2_hashmap_size;
 * level_offset = prefix sum of the rows owned: (R_l + 1)^3 for a dense level, T for a hashed one; level_offset[n_levels] =
 * rows_total) and computes none of them.  The record lives in host memory.
 *   slot of node (ix, iy, iz):  dense   ix + iy (R + 1) + iz (R + 1)^2
 *                               hashed  (ix ^ iy * 2654435761 ^ iz * 805459861) mod T     in wrapping uint32 arithmetic
 *   per point and level, in fp32 without contraction:  u = clamp((x - lo) inv_extent, 0, 1),  p = u R,  i = min(int(floor(p)), R - 1),
 *   f = p - i;  corner c (bit 0 x, bit 1 y, bit 2 z) has the weight (wx wy) wz, wx = c & 1 ? fx : 1 - fx, ..;
 *   out[p][l F + k] = sum_c w_c E[level_offset[l] + slot_c][k], accumulated in ascending c from w_0 v_0.
 * Points outside the box are clamped; a non-finite coordinate reads inside the table (its output is unspecified).
 * The points are either `points` [n_points][3], or -- points NULL -- o + d z_vals of ray records [n_points / n_samples][ray_stride]
 * (o3, d3, ..) and z_vals [n_points], a separate multiply and add as in nerf_build_inputs.
 *   nerf_hash_encode_fwd: writes columns 0 .. L F of the row-major matrix `out` with leading dimension ld_out >= L F (point it at a
 *     column of a wider matrix: the other columns are untouched).  n_points == 0 returns 0 and launches nothing.
 *   nerf_hash_encode_bwd: d_embeddings [rows_total][F], every element written, from d_out [n_points][ld_d_out]; deterministic.  With
 *     M = max |d_out| = m 2^e (frexp) found on the device and q = 61 - e - ceil(log2(max(n_points, 1))), every contribution
 *     t = w_c g (one fp32 product) becomes k = llrint((double)t 2^q) and is added to scratch[row][k] by a 64-bit integer atomic add;
 *     the finishing pass writes (float)((double)acc 2^-q) and zeroes the accumulator.  |sum| <= M P < 2^61: no overflow, and integer
 *     addition does not depend on its order, so two calls give the same bits.  M == 0: all zeros.  M not finite: all NaN (decided on
 *     the device, no host read-back).  scratch: nerf_hash_scratch_words(grid) 64-bit words, 8-byte aligned, ZERO before its first use;
 *     a complete call (phases = 3, or 1 then 2) leaves the accumulator zero (the last word holds the bits of M and is rewritten by every call).  phases: 1 = the maximum and the scatter, 2 = the finishing pass,
 *     3 = both (1 and 2 as two calls with the same arguments give the bits of 3; they exist so the two can be timed apart).
 *     No gradient with respect to the points is computed by this entry point.
 *   nerf_hash_input_grad (csrc/hash_input_grad.hip): the gradient with respect to the POINTS, a gather of the forward's
 *     rows with the forward's cell, weights and slots.  d_x [n_points][ld_d_x] holds dL/d(encoding) in columns 0 .. L F.  Per point
 *     and level, in fp32 without contraction:  v_c = sum_k d_x[p][l F + k] E[row_c][k] (k ascending from the first product);
 *     df_x = sum_c +-((wy wz) v_c), + where bit 0 of c is set, accumulated in ascending c from -((wy wz) v_0); df_y with (wx wz) and
 *     bit 1, df_z with (wx wy) and bit 2;  g_a = sum_l (df_a R_l) inv_extent[a] in ascending l from 0, a level's term replaced by an
 *     exact 0 on an axis whose unclamped t = (x - lo) inv_extent is < 0 or > 1 (on the faces: the derivative of the cell the forward
 *     picks).  Point mode (`points` given): writes d_points [n_points][3]; d_rays, workspace NULL, views_col = -1, accumulate = 0.
 *     Ray mode (`rays` + z_vals): two launches -- the same lane-per-point kernel into `workspace` (the workspace_floats function below:
 *     3 n_points floats), then one wavefront per ray: lane j takes samples j, j + 64, .. in ascending order, a fixed xor butterfly (32,
 *     16, .., 1) -- and writes d_rays [n_rays][11] by nerf_field_input_grad's column contract: 0:3 = sum_s g_s, 3:6 = sum_s z_s g_s (one
 *     fp32 product each), 6:8 = 0, 8:11 = the adjoint of the view columns [v, sin 2^0 v, cos 2^0 v, ..] (3 + 6 multires_views columns
 *     of d_x from views_col on, as nerf_build_inputs writes them; multires_views = -1: the identity's 3) applied once to the column
 *     sums over the ray's samples, or 0 when views_col < 0.  z_vals, near and far are constants.  accumulate != 0 adds to d_rays and
 *     leaves columns 6:8 alone.  No atomics: two calls give the same bits; with n_samples = 1 columns 0:3 are point mode's bits.
 *     A non-finite coordinate reads inside the table; its own row of the output is unspecified.  n_points == 0 launches nothing. */
#define NERF_HASH_MAX_LEVELS 32
typedef struct NerfHashGrid {
    int n_levels, n_features, log2_hashmap_size, reserved;
    float lo[3], inv_extent[3];
    int level_resolution[NERF_HASH_MAX_LEVELS];
    int level_dense[NERF_HASH_MAX_LEVELS];
    long long level_offset[NERF_HASH_MAX_LEVELS + 1];
} NerfHashGrid;
size_t nerf_hash_scratch_words(const NerfHashGrid* grid);
int nerf_hash_encode_fwd(const NerfHashGrid* grid, const float* embeddings, const float* points /* nullable */, const float* rays /* nullable */,
                         int ray_stride, const float* z_vals /* nullable */, int n_samples, long n_points, float* out, int ld_out, void* stream);
int nerf_hash_encode_bwd(const NerfHashGrid* grid, const float* points /* nullable */, const float* rays /* nullable */, int ray_stride,
                         const float* z_vals /* nullable */, int n_samples, long n_points, const float* d_out, int ld_d_out, long long* scratch,
                         float* d_embeddings, int phases, void* stream);
size_t nerf_hash_input_grad_workspace_floats(long n_points);
int nerf_hash_input_grad(const NerfHashGrid* grid, const float* embeddings, const float* points /* nullable */, const float* rays /* nullable */,
                         int ray_stride, const float* z_vals /* nullable */, int n_samples, long n_points, const float* d_x, int ld_d_x,
                         int views_col, int multires_views, float* d_points /* point mode */, float* d_rays /* ray mode */,
                         float* workspace /* ray mode */, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif

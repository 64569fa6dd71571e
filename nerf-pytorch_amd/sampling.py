"""Device-side ray-batch sampling for train().

The reference builds a full [H, W, 3] ray grid per step, a meshgrid of pixel coordinates and draws
``np.random.choice(H*W, N_rand, replace=False)`` on the host, then copies one image host->device
(run_nerf.py:730-757).  At fused-kernel speed that host work (an O(H*W) permutation, ~10 ms at 800x800) would cap
rays/s, so here everything stays on the device and rays are generated ONLY for the selected pixels:

    batch_rays, target_s = sample_ray_batch(H, W, K, pose, image, N_rand, precrop_frac=...)

returns exactly what train() feeds to render(): ``batch_rays [2, N_rand, 3]`` (rays_o, rays_d as get_rays would
give them for those pixels, run_nerf_helpers.py:153-162) and ``target_s [N_rand, 3]``.  Selection is uniform without
replacement like the reference's.  On the GPU it is ONE launch of N_rand threads (nerf_sample_ray_batch: pixel k = a keyed
bijection of the window's pixel range applied to k -- distinct by construction, no O(H*W) permutation, no device sort), keyed by
two words drawn per step from the HOST generator (torch's default CPU generator, i.e. torch.manual_seed, or a CPU
``generator=``): no device synchronisation.  CPU tensors take the torch formulation (tests of the bookkeeping).

A ``pose`` that requires grad keeps ``batch_rays`` in the graph: their backward is nerf_ray_pose_grad, the adjoint of the ray set-up
(pose refinement).  ``RayBatcher`` is the device form of the reference's ``use_batching`` mode (run_nerf.py:676-726): batches of
N_rand rays over the pixels of ALL training views, drawn from the pose table passed at each step (a refined pose table works).
"""
import numpy as np
import torch

from . import hip_backend as hb


def _window(H, W, precrop_frac):
    if precrop_frac is not None:
        dH, dW = int(H // 2 * precrop_frac), int(W // 2 * precrop_frac)
        return H // 2 - dH, W // 2 - dW, 2 * dH, 2 * dW
    return 0, 0, H, W


def _draw_key(generator):
    """two key words from the host generator (a device generator works too: its draw is read back, one synchronisation)"""
    gdev = generator.device if generator is not None else torch.device("cpu")
    return torch.randint(0, 2 ** 31 - 1, (2,), generator=generator, device=gdev).tolist()


def _pose_grad_like(shape, d):
    """d [.., 3, 4] -> a gradient of `shape` ([.., 3, 4] or [.., 4, 4]: row 3 gets zeros)"""
    if tuple(shape[-2:]) == (3, 4):
        return d.reshape(shape)
    g = d.new_zeros(shape)
    g[..., :3, :4] = d
    return g


class _PoseRays(torch.autograd.Function):
    """nerf_sample_ray_batch with batch_rays as a function of the pose; backward: nerf_ray_pose_grad at the selected pixels"""

    @staticmethod
    def forward(ctx, c2w, H, W, K, image, N_rand, window, key):
        rays, target, pix = hb.sample_ray_batch(H, W, K, c2w, image, N_rand, window, key, want_pixels=True)
        ctx.save_for_backward(pix)
        ctx.W, ctx.K, ctx.shape = W, K, c2w.shape
        ctx.mark_non_differentiable(target, pix)
        return rays, target, pix

    @staticmethod
    def backward(ctx, d_rays, _d_target, _d_pix):
        pix, = ctx.saved_tensors
        d = hb.ray_pose_grad(ctx.W, ctx.K, d_rays.float(), pix, None, 1)
        return (_pose_grad_like(ctx.shape, d[0]),) + (None,) * 7


class _ViewRays(torch.autograd.Function):
    """nerf_sample_ray_views with batch_rays as a function of the pose table; backward: nerf_ray_pose_grad per view, scattered into
    the table's rows of the training views (the others get zeros)"""

    @staticmethod
    def forward(ctx, poses, H, W, K, view_ids, images, N_rand, batch, key):
        rays, target, pix, views = hb.sample_ray_views(H, W, K, view_ids, poses, images, N_rand, batch, key, want_pixels=True, want_views=True)
        ctx.save_for_backward(pix, views, view_ids)
        ctx.W, ctx.K, ctx.shape = W, K, poses.shape
        ctx.mark_non_differentiable(target, pix, views)
        return rays, target, pix, views

    @staticmethod
    def backward(ctx, d_rays, _d_target, _d_pix, _d_views):
        pix, views, view_ids = ctx.saved_tensors
        d = hb.ray_pose_grad(ctx.W, ctx.K, d_rays.float(), pix, views, view_ids.numel())
        g = d.new_zeros(ctx.shape)
        g[view_ids.long(), :3, :4] = d          # (the view list holds no index twice: RayBatcher checks)
        return (g,) + (None,) * 8


def sample_ray_batch(H, W, K, pose, image, N_rand, precrop_frac=None, generator=None, return_pixels=False):
    """pose [3,4] or [4,4] camera-to-world, image [H,W,3] (device tensors).  precrop_frac: central crop used during
    the first precrop_iters steps (run_nerf.py:738-747).  generator: a CPU torch.Generator (default: torch's global CPU generator)
    for the sync-free kernel path; a device generator works too (its draw is read back: one synchronisation).
    A pose that requires grad (grad mode on) gets d loss / d pose through batch_rays (nerf_ray_pose_grad; a [4,4] pose's row 3 gets
    zeros); target_s is not differentiable.  Otherwise the outputs and launches are those of the plain sampler."""
    dev = image.device
    h0, w0, nh, nw = _window(H, W, precrop_frac)
    if N_rand > nh * nw:        # np.random.choice(..., replace=False) raises here too (run_nerf.py:752)
        raise ValueError(f"cannot take N_rand={N_rand} rays without replacement from {nh}x{nw} = {nh * nw} pixels")
    if image.is_cuda:
        key = _draw_key(generator)
        img = image if image.dtype == torch.float32 and image.is_contiguous() else image.float().contiguous()
        if isinstance(pose, torch.Tensor) and pose.requires_grad and torch.is_grad_enabled():
            c2w = pose.to(dev, torch.float32)
            c2w = c2w if c2w.stride(-1) == 1 else c2w.contiguous()
            rays, target, pix = _PoseRays.apply(c2w, H, W, K, img, N_rand, (h0, w0, nh, nw), key)
            return (rays, target, pix) if return_pixels else (rays, target)
        c2w = pose if (isinstance(pose, torch.Tensor) and pose.is_cuda and pose.dtype == torch.float32 and pose.stride(-1) == 1) \
            else torch.as_tensor(pose, dtype=torch.float32).to(dev).contiguous()
        out = hb.sample_ray_batch(H, W, K, c2w, img, N_rand, (h0, w0, nh, nw), key, want_pixels=return_pixels)
        return out
    sel = torch.randperm(nh * nw, device=dev, generator=generator)[:N_rand]
    jj = h0 + torch.div(sel, nw, rounding_mode="floor")      # row (y)
    ii = w0 + sel - torch.div(sel, nw, rounding_mode="floor") * nw      # column (x)
    i = ii.to(torch.float32)
    j = jj.to(torch.float32)
    dirs = torch.stack([(i - K[0][2]) / K[0][0], -(j - K[1][2]) / K[1][1], -torch.ones_like(i)], -1)
    c2w = pose[:3, :4].to(dev)
    rays_d = torch.sum(dirs[..., None, :] * c2w[:3, :3], -1)
    rays_o = c2w[:3, -1].expand(rays_d.shape)
    target_s = image[jj, ii]
    out = (torch.stack([rays_o, rays_d], 0), target_s)
    return out + ((jj * W + ii).to(torch.int32),) if return_pixels else out


class RayBatcher:
    """The reference's ``use_batching`` mode (no_batching = False, the default; run_nerf.py:676-726) on the device.

    The reference builds rays_rgb [V*H*W, 3, 3] once on the host with get_rays_np, shuffles it with numpy, and takes consecutive
    N_rand windows, reshuffling after each epoch: 36 bytes per ray, built for poses that never change.  Here nothing is built: batch b of
    epoch e is positions [b*N_rand, min((b+1)*N_rand, V*H*W)) of a keyed bijection of the (view, pixel) space of ``i_train``
    (nerf_sample_ray_views, one launch), and the rays are made from the pose table passed to :meth:`next`, so a pose table that is
    being refined (requires grad) is used as it stands that step and receives d loss / d poses (nerf_ray_pose_grad).  The last batch of an
    epoch is short, as the reference's slice is; then a new epoch with a new order starts.

    Each epoch draws its two key words from the HOST generator (``generator``: a CPU torch.Generator, default torch's global one): no
    device synchronisation.  Like sample_ray_batch this cannot reproduce np.random.shuffle's stream: the order is a different uniform
    shuffle.  CPU tensors take a torch.randperm formulation (the same bookkeeping, for tests without a GPU).

        batcher = RayBatcher(images, K, N_rand, i_train)
        batch_rays, target_s = batcher.next(poses)          # poses [N, 3|4, 4]: the whole table, indexed by i_train
    """

    def __init__(self, images, K, N_rand, i_train, generator=None):
        if not (isinstance(images, torch.Tensor) and images.dim() == 4 and images.shape[-1] == 3):
            raise ValueError("images must be a [N, H, W, 3] tensor")
        if images.is_cuda and not (images.dtype == torch.float32 and images[0].is_contiguous()):
            images = images.float().contiguous()
        self.images, self.K, self.N_rand, self.generator = images, K, int(N_rand), generator
        self.H, self.W = int(images.shape[1]), int(images.shape[2])
        ids = torch.as_tensor(np.asarray(i_train.cpu() if isinstance(i_train, torch.Tensor) else i_train), dtype=torch.int64).reshape(-1)
        if ids.numel() == 0 or int(ids.min()) < 0 or int(ids.max()) >= images.shape[0]:
            raise ValueError(f"i_train must hold view indices in [0, {images.shape[0]})")
        if torch.unique(ids).numel() != ids.numel():
            raise ValueError("i_train holds a view twice")
        if self.N_rand <= 0:
            raise ValueError("N_rand must be positive")
        self.n_rays = ids.numel() * self.H * self.W
        if images.is_cuda and self.n_rays >= 2 ** 32:
            raise ValueError(f"V*H*W = {self.n_rays} rays: the device sampler indexes the (view, pixel) space with 32 bits")
        self.view_ids = ids.to(images.device, torch.int32 if images.is_cuda else torch.int64)
        self.epoch, self.i_batch = 0, 0
        self._start_epoch()

    def _start_epoch(self):
        if self.images.is_cuda:
            self._key = _draw_key(self.generator)
        else:
            self._perm = torch.randperm(self.n_rays, generator=self.generator)

    def next(self, poses, return_pixels=False, return_views=False):
        """(batch_rays [2, B, 3], target_s [B, 3]) of the next batch, rays from ``poses`` [N, 3|4, 4] (the whole pose table; the
        rows of i_train are read).  return_pixels / return_views append pixels [B] (j*W + i) / views [B] (position in i_train)."""
        dev = self.images.device
        if self.images.is_cuda:
            key, batch = self._key, self.i_batch // self.N_rand
            if isinstance(poses, torch.Tensor) and poses.requires_grad and torch.is_grad_enabled():
                c2w = poses.to(dev, torch.float32)
                c2w = c2w if c2w.stride(-1) == 1 else c2w.contiguous()
                rays, target, pix, views = _ViewRays.apply(c2w, self.H, self.W, self.K, self.view_ids, self.images, self.N_rand, batch, key)
            else:
                c2w = torch.as_tensor(poses).detach().to(dev, torch.float32)
                c2w = c2w if c2w.stride(-1) == 1 else c2w.contiguous()
                rays, target, pix, views = hb.sample_ray_views(self.H, self.W, self.K, self.view_ids, c2w, self.images, self.N_rand, batch,
                                                               key, want_pixels=return_pixels, want_views=return_views)
        else:
            q = self._perm[self.i_batch:self.i_batch + self.N_rand]
            hw = self.H * self.W
            views = torch.div(q, hw, rounding_mode="floor")
            pix = q - views * hw
            jj = torch.div(pix, self.W, rounding_mode="floor")
            ii = pix - jj * self.W
            t = self.view_ids[views]
            K = self.K
            i, j = ii.to(torch.float32), jj.to(torch.float32)
            dirs = torch.stack([(i - K[0][2]) / K[0][0], -(j - K[1][2]) / K[1][1], -torch.ones_like(i)], -1)
            c2w = torch.as_tensor(poses)[t, :3, :4]
            rays_d = torch.sum(dirs[..., None, :] * c2w[:, :3, :3], -1)
            rays_o = c2w[:, :3, -1]
            rays, target = torch.stack([rays_o, rays_d], 0), self.images[t, jj, ii]
            pix, views = pix.to(torch.int32), views.to(torch.int32)
        self.i_batch += target.shape[0]
        if self.i_batch >= self.n_rays:         # run_nerf.py:721-726: reshuffle after an epoch
            self.epoch += 1
            self.i_batch = 0
            self._start_epoch()
        out = (rays, target)
        if return_pixels:
            out += (pix,)
        if return_views:
            out += (views,)
        return out

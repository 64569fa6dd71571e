"""Camera-pose refinement (NeRF--, BARF style): a learnable se(3) correction per view.

    refine = PoseRefinement(len(poses)).to(dev)
    batch_rays, target_s = batcher.next(refine(poses))      # sampling.RayBatcher; d loss / d xi flows back through the rays

Small host-side glue on [V, 6]: batched torch ops, no kernel.  The gradient path from the rays to the pose table is
nerf_ray_pose_grad (sampling.py) or render()'s own ray set-up (render(c2w=...)).
"""
import torch


def se3_exp(xi):
    """[V, 6] twists (omega, v) -> [V, 4, 4] exp of the twist matrix [[omega]_x, v; 0, 0] (torch.linalg.matrix_exp: smooth at 0)"""
    w, v = xi[:, :3], xi[:, 3:]
    z = torch.zeros_like(w[:, 0])
    A = torch.stack([torch.stack([z, -w[:, 2], w[:, 1], v[:, 0]], -1),
                     torch.stack([w[:, 2], z, -w[:, 0], v[:, 1]], -1),
                     torch.stack([-w[:, 1], w[:, 0], z, v[:, 2]], -1),
                     torch.stack([z, z, z, z], -1)], -2)
    return torch.linalg.matrix_exp(A)


class PoseRefinement(torch.nn.Module):
    """xi [n_views, 6], zero-initialised; forward(poses [n_views, 3|4, 4]) = exp(xi_v) @ pose_v (same shape as poses).  A table with
    views that are never sampled is fine: their xi get exact zero gradients, and Adam leaves them at 0."""

    def __init__(self, n_views):
        super().__init__()
        self.xi = torch.nn.Parameter(torch.zeros(int(n_views), 6))

    def forward(self, poses):
        if poses.dim() != 3 or poses.shape[0] != self.xi.shape[0] or tuple(poses.shape[1:]) not in ((3, 4), (4, 4)):
            raise ValueError(f"poses must be [{self.xi.shape[0]}, 3|4, 4], got {tuple(poses.shape)}")
        T = se3_exp(self.xi).to(poses.dtype)
        P = poses if poses.shape[1] == 4 else torch.cat([poses, poses.new_tensor([0.0, 0.0, 0.0, 1.0]).expand(len(poses), 1, 4)], 1)
        return (T @ P)[:, :poses.shape[1]]

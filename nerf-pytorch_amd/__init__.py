"""nerf-pytorch_amd: MI355X (gfx950) implementation of the nerf-pytorch render hot path.

Drop-in surface (same names / signatures as the reference's run_nerf.py and
run_nerf_helpers.py): ``render``, ``render_path``, ``render_rays``, ``batchify_rays``,
``raw2outputs``, ``run_network``, ``sample_pdf``, ``Embedder``, ``get_embedder``, ``NeRF``,
``create_nerf``, ``config_parser``.  The directory name carries a hyphen (contract of
this build); import it as ``nerf_pytorch_amd`` (root-level shim module).
"""
from .field import Embedder, NeRF, get_embedder  # noqa: F401
from .render import (batchify, batchify_rays, get_rays, get_rays_np, img2mse, mse2psnr, ndc_rays,  # noqa: F401
                     query_points, raw2outputs, render, render_path, render_rays, run_network, sample_pdf, to8b,
                     set_precision, get_precision, check_range, DEFAULT_PRECISION, distortion_loss, distortion_loss_reference,
                     interlevel_loss, interlevel_loss_reference)
from .nerf_setup import config_parser, create_nerf  # noqa: F401
from . import hip_backend, parallel  # noqa: F401
from .optim import FlatAdam  # noqa: F401
from .sampling import RayBatcher, sample_ray_batch  # noqa: F401
from .pose import PoseRefinement  # noqa: F401
from .occupancy import DensityGrid, OccupancyGrid  # noqa: F401
from . import occupancy  # noqa: F401
from .mesh import density_volume, extract_mesh, extract_mesh_reference, mesh_from_network, write_ply  # noqa: F401
from . import mesh  # noqa: F401
from .baked import BakedField, BakedTrainer, ray_records, regularizer_reference, sh_basis  # noqa: F401
from . import baked  # noqa: F401
from .hashgrid import HashEncoding, HashNeRF  # noqa: F401
from . import hashgrid  # noqa: F401

__all__ = ["density_volume", "extract_mesh", "extract_mesh_reference", "mesh_from_network", "write_ply", "mesh","Embedder", "NeRF", "get_embedder", "batchify", "batchify_rays", "get_rays", "get_rays_np", "img2mse",
           "mse2psnr", "ndc_rays", "query_points", "raw2outputs", "render", "render_path", "render_rays",
           "run_network", "sample_pdf", "to8b", "config_parser", "create_nerf", "hip_backend", "parallel", "set_precision", "get_precision", "FlatAdam", "sample_ray_batch", "RayBatcher", "PoseRefinement", "DEFAULT_PRECISION", "check_range", "OccupancyGrid", "DensityGrid", "occupancy",
           "distortion_loss", "distortion_loss_reference", "interlevel_loss", "interlevel_loss_reference", "BakedField", "BakedTrainer", "sh_basis", "baked", "regularizer_reference", "ray_records",
           "HashEncoding", "HashNeRF", "hashgrid"]

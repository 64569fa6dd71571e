"""CPU: the argument guards of the dense-layer entry points (csrc/dense.hip: nerf_dense_fwd / _dgrad / _wgrad, nerf_build_inputs).
Every call here is one a guard refuses -- NERF_E_BADARG (-1) and a nerf_last_error() that names the entry point and the reason --
before rocBLAS is loaded or anything is launched, so fake non-null addresses are enough (nothing is dereferenced)."""
import pytest

import nerf_pytorch_amd as npa

X, W, Y, B, S = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000        # fake device addresses


def _refused(name, args, reason):
    L = npa.hip_backend.lib()
    assert L.nerf_pack_params(None, None, None) == -1 and b"nerf_pack_params" in L.nerf_last_error()      # another call's message first
    assert getattr(L, name)(*args) == -1, (name, args)
    err = L.nerf_last_error()
    assert err.startswith(name.encode() + b": ") and reason in err, (name, args, err)


def _with(base, **changes):
    return tuple({**base, **changes}.values())


# argument lists in the order of include/nerf_hip.h (dicts keep insertion order); each base call would be valid with real memory
FWD = dict(x=X, ldx=9, K=4, w=W, ldw=6, bias=B, y=Y, ldy=8, N=5, P=7, accumulate=0, relu=1, stream=None)
DGRAD = dict(dy=Y, lddy=8, N=5, w=W, ldw=6, dx=X, lddx=9, K=4, P=7, accumulate=0, act=B, ldact=7, stream=None)
WGRAD = dict(dy=Y, lddy=8, N=5, x=X, ldx=9, K=4, P=7, dw=W, lddw=6, dbias=B, scratch=S, accumulate=0, stream=None)
BUILD = dict(rays=X, ray_stride=11, z_vals=Y, n_rays=3, n_samples=5, multires=10, multires_views=4, use_viewdirs=1, x=W, ldx=90, stream=None)
ROWS_TOO_MANY = 1 << 31         # P must fit an int: 2^31 - 1 is the last accepted value


@pytest.mark.parametrize("name,base,required", [("nerf_dense_fwd", FWD, ("x", "w", "y")), ("nerf_dense_dgrad", DGRAD, ("dy", "w", "dx")),
                                                ("nerf_dense_wgrad", WGRAD, ("dy", "x", "dw")),
                                                ("nerf_build_inputs", BUILD, ("rays", "z_vals", "x"))])
def test_each_required_pointer_is_checked(name, base, required):
    for arg in required:
        _refused(name, _with(base, **{arg: None}), b"null pointer")
    _refused(name, _with(base, **dict.fromkeys(required)), b"null pointer")


@pytest.mark.parametrize("name,base", [("nerf_dense_fwd", FWD), ("nerf_dense_dgrad", DGRAD), ("nerf_dense_wgrad", WGRAD)])
def test_sizes_of_the_gemm_entry_points(name, base):
    for change in (dict(K=0), dict(K=-3), dict(N=0), dict(N=-1), dict(P=-1), dict(P=ROWS_TOO_MANY), dict(P=ROWS_TOO_MANY + 5)):
        _refused(name, _with(base, **change), b"bad size")
    # a bad size is refused for the empty batch too, and the matrices that are not row operands stay required there
    _refused(name, _with(base, P=0, K=0), b"bad size")
    _refused(name, _with(base, P=0, **{"dw" if name == "nerf_dense_wgrad" else "w": None}), b"null pointer")


def test_leading_dimensions_smaller_than_the_width():
    for ld, width in (("ldx", "K"), ("ldw", "K"), ("ldy", "N")):
        _refused("nerf_dense_fwd", _with(FWD, **{ld: FWD[width] - 1}), b"leading dimension")
        _refused("nerf_dense_fwd", _with(FWD, **{ld: 0}), b"leading dimension")
        _refused("nerf_dense_fwd", _with(FWD, P=0, **{ld: FWD[width] - 1}), b"leading dimension")
    for ld, width in (("lddy", "N"), ("ldw", "K"), ("lddx", "K"), ("ldact", "K")):
        _refused("nerf_dense_dgrad", _with(DGRAD, **{ld: DGRAD[width] - 1}), b"leading dimension")
        _refused("nerf_dense_dgrad", _with(DGRAD, P=0, **{ld: DGRAD[width] - 1}), b"leading dimension")
    _refused("nerf_dense_dgrad", _with(DGRAD, ldact=0), b"leading dimension")         # (ldact is read only when act is given)
    for ld, width in (("lddy", "N"), ("ldx", "K"), ("lddw", "K")):
        _refused("nerf_dense_wgrad", _with(WGRAD, **{ld: WGRAD[width] - 1}), b"leading dimension")
        _refused("nerf_dense_wgrad", _with(WGRAD, P=0, **{ld: WGRAD[width] - 1}), b"leading dimension")
    # K and N are not interchangeable: a leading dimension that fits the other width only
    _refused("nerf_dense_fwd", _with(FWD, K=5, N=4, ldx=4), b"leading dimension")
    _refused("nerf_dense_dgrad", _with(DGRAD, K=5, N=4, lddx=4, ldact=9), b"leading dimension")
    _refused("nerf_dense_wgrad", _with(WGRAD, K=5, N=4, lddw=4), b"leading dimension")


def test_bias_gradient_without_scratch():
    _refused("nerf_dense_wgrad", _with(WGRAD, scratch=None), b"scratch")
    _refused("nerf_dense_wgrad", _with(WGRAD, scratch=None, accumulate=1), b"scratch")


def test_sizes_of_build_inputs():
    for change in (dict(n_samples=0), dict(n_samples=-2), dict(n_rays=-1), dict(multires=25), dict(multires_views=25),
                   dict(multires=1 << 20), dict(n_rays=0, n_samples=0), dict(n_rays=0, multires=25)):
        _refused("nerf_build_inputs", _with(BUILD, **change), b"bad size")
    # ldx below the encoded width: 63 + 27 with view directions, 63 without; 3 + 3 for the identity embeddings; 3 + 0 bands = 3
    _refused("nerf_build_inputs", _with(BUILD, ldx=89), b"bad size")
    _refused("nerf_build_inputs", _with(BUILD, use_viewdirs=0, ray_stride=8, ldx=62), b"bad size")
    _refused("nerf_build_inputs", _with(BUILD, multires=-1, multires_views=-1, ldx=5), b"bad size")
    _refused("nerf_build_inputs", _with(BUILD, multires=0, multires_views=0, ldx=5), b"bad size")
    _refused("nerf_build_inputs", _with(BUILD, multires=24, multires_views=24, ldx=2 * 147 - 1), b"bad size")
    _refused("nerf_build_inputs", _with(BUILD, n_rays=0, ldx=89), b"bad size")
    # ray records: o3 d3 near far [viewdir3]
    _refused("nerf_build_inputs", _with(BUILD, use_viewdirs=0, ray_stride=7, ldx=63), b"bad size")
    _refused("nerf_build_inputs", _with(BUILD, use_viewdirs=0, ray_stride=0, ldx=63), b"bad size")
    _refused("nerf_build_inputs", _with(BUILD, ray_stride=10), b"bad size")
    _refused("nerf_build_inputs", _with(BUILD, ray_stride=8), b"bad size")

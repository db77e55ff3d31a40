"""CPU-side checks of FaceNeRF.forward with gradients: the new C entries reject bad arguments before touching a device,
and the module path refuses CPU tensors instead of falling back.  No GPU needed."""
import ctypes as C

import pytest
import torch

import oracle


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    return idealnerf_amd


def _fake_params(idn, dims=(64, 76, 32)):
    """Non-NULL addresses that are never dereferenced: argument checks return before any launch."""
    L = idn._lib
    p, g = L.FaceNerfParams(), L.FaceNerfGrads()
    for i in range(8):
        p.pts_w[i] = p.pts_b[i] = g.pts_w[i] = g.pts_b[i] = 256
    for i in range(3):
        p.views_w[i] = p.views_b[i] = g.views_w[i] = g.views_b[i] = 256
    p.alpha_w = p.alpha_b = p.rgb_w = p.rgb_b = g.alpha_w = g.alpha_b = g.rgb_w = g.rgb_b = 256
    p.dim_aud, p.dim_expr, p.dim_latent = dims
    return p, g


def test_facenerf_train_fwd_argument_errors(idn):
    lib = idn._lib.load()
    F = 256   # any non-NULL address
    assert lib.idealnerf_facenerf_train_fwd(F, F, idn._lib.IDN_PREC_BF16X3, F, 8, F, F, None) == -2   # not fp32-grade
    assert lib.idealnerf_facenerf_train_fwd(F, F, idn._lib.IDN_PREC_BF16, F, 8, F, F, None) == -2
    assert lib.idealnerf_facenerf_train_fwd(F, F, idn._lib.IDN_PREC_F32, F, -1, F, F, None) == -1
    assert lib.idealnerf_facenerf_train_fwd(F, F, idn._lib.IDN_PREC_BF16X6, F, 8, F, None, None) == -1   # acts NULL
    assert b"NULL" in lib.idealnerf_last_error()
    assert lib.idealnerf_facenerf_train_fwd(None, F, idn._lib.IDN_PREC_F32, F, 8, F, F, None) == -1
    assert lib.idealnerf_facenerf_train_fwd(None, None, idn._lib.IDN_PREC_F32, None, 0, None, None, None) == 0   # nothing to do


def test_facenerf_bwd_argument_errors(idn):
    lib = idn._lib.load()
    F = 256
    p, g = _fake_params(idn)
    args = lambda **kw: dict(dict(aud=F, expr=F, latent=F, acts=F, n=8, g_out=F), **kw)

    def call(p_=C.byref(p), g_=C.byref(g), **kw):
        a = args(**kw)
        return lib.idealnerf_facenerf_bwd(p_, g_, a["aud"], a["expr"], a["latent"], a["acts"], a["n"], a["g_out"], None, None,
                                          None, None, None, 0, None)

    assert call(p_=None) == -1
    assert call(g_=None) == -1
    assert call(p_=C.byref(idn._lib.FaceNerfParams())) == -1   # NULL parameter tensors
    g0 = idn._lib.FaceNerfGrads()
    assert call(g_=C.byref(g0)) == -1                          # NULL gradient tensors
    assert call(n=-1) == -1
    assert call(acts=None) == -1
    assert call(g_out=None) == -1
    assert call(expr=None) == -1                               # dim_expr = 76 needs expr
    assert call(n=0) == 0
    # the workspace is the render pass's for the same number of points
    assert lib.idealnerf_facenerf_bwd_workspace_bytes(0) == 0
    for n in (1, 128, 40000):
        assert lib.idealnerf_facenerf_bwd_workspace_bytes(n) == lib.idealnerf_pass_bwd_workspace_bytes(n, 1) > 0


def test_module_with_gradients_refuses_cpu_tensors(idn):
    """A FaceNeRF left on the CPU, called with gradients on: IdealNerfError (no eager fallback), not NotImplementedError --
    and the same when only a conditioning vector requires grad."""
    dims = oracle.facenerf_dims()
    net = idn.FaceNeRF(dim_aud=64, dim_latent=32, dim_expr=76)
    net.load_state_dict(oracle.xavier_facenerf_params(1, dims))
    x = torch.rand(4, 90)
    aud, expr, lat = torch.zeros(64), torch.zeros(76), torch.zeros(32)
    with pytest.raises(idn._lib.IdealNerfError, match="GPU"):
        net(x, aud, expr, lat)
    net.requires_grad_(False)
    with pytest.raises(idn._lib.IdealNerfError, match="GPU"):
        net(x, aud, expr, lat.requires_grad_(True))
    lib = idn._lib.load()
    packed = torch.zeros(lib.idealnerf_packed_weight_floats(idn._lib.IDN_PREC_BF16X6))
    with pytest.raises(idn._lib.IdealNerfError, match="GPU"):
        idn.ops.facenerf_train_fwd(packed, torch.zeros(lib.idealnerf_folded_bias_floats()), x, idn._lib.IDN_PREC_BF16X6)

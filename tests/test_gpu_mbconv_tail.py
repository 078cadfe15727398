"""GPU: K12, the squeeze-excite gate of an MBConv block in one launch (csrc/se.hip), against an fp64
torch evaluation, and the folded EfficientNetV2-S forward that uses it against the unfused folded path."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (C, S): EfficientNetV2-S stages 4-6, EfficientNetV2-L stages 4-7, MobileNetV3-Large's SE blocks
SHAPES_S = [(256, 16), (512, 32), (768, 32), (960, 40), (1536, 64)]
SHAPES_L = [(384, 24), (768, 48), (1152, 48), (1344, 56), (2304, 96), (3840, 160)]
SHAPES_MBV3 = [(72, 18), (120, 30), (480, 120), (672, 168), (960, 240)]


def _se_inputs(B, C, S, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    mean = torch.randn(B, C, device='cuda', generator=g)
    w1 = torch.randn(S, C, 1, 1, device='cuda', generator=g) / C ** 0.5
    b1 = 0.1 * torch.randn(S, device='cuda', generator=g)
    w2 = torch.randn(C, S, 1, 1, device='cuda', generator=g) / S ** 0.5
    b2 = 0.1 * torch.randn(C, device='cuda', generator=g)
    return mean, w1, b1, w2, b2


def _se_fp64(mean, w1, b1, w2, b2, act, gate):
    d = lambda t: t.double()
    h = d(mean) @ d(w1).flatten(1).T + d(b1)
    h = F.silu(h) if act == 'silu' else F.relu(h)
    z = h @ d(w2).flatten(1).T + d(b2)
    return torch.sigmoid(z) if gate == 'sigmoid' else F.hardsigmoid(z)


@pytest.mark.parametrize('act,gate', [('silu', 'sigmoid'), ('relu', 'hardsigmoid'), ('silu', 'hardsigmoid'),
                                      ('relu', 'sigmoid')])
@pytest.mark.parametrize('B', [1, 3, 64])
def test_se_gate_matches_fp64(act, gate, B, hip_lib):
    from metrabs_amd import kernels
    for i, (C, S) in enumerate(SHAPES_S + SHAPES_L + SHAPES_MBV3):
        args = _se_inputs(B, C, S, 100 + i)
        got = kernels.se_gate(*args, act, gate)
        ref = _se_fp64(*args, act, gate)
        assert got.shape == (B, C) and got.dtype == torch.float32
        err = float((got.double() - ref).abs().max())
        assert err <= 1e-5, (C, S, B, err)   # gates in [0, 1]; f32 sums over up to 3840 terms


def test_se_gate_is_deterministic_and_graph_safe(hip_lib):
    from metrabs_amd import kernels
    args = _se_inputs(64, 1536, 64, 7)
    a = kernels.se_gate(*args, 'silu', 'sigmoid')
    b = kernels.se_gate(*args, 'silu', 'sigmoid')
    assert torch.equal(a, b)
    with torch.inference_mode():   # (as the model is captured: the other graph tests' setting)
        out = torch.empty_like(a)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            kernels.se_gate(*args, 'silu', 'sigmoid', out=out)
            st.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                kernels.se_gate(*args, 'silu', 'sigmoid', out=out)
        torch.cuda.current_stream().wait_stream(st)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, a)


def test_se_gate_entry_point_rejects_null_and_bad_shapes(hip_lib):
    from metrabs_amd import _lib
    null = ctypes.c_void_p(0)
    t = torch.zeros(64, device='cuda')
    p = ctypes.c_void_p(t.data_ptr())
    assert hip_lib.mtr_se_gate(null, p, p, p, p, 2, 0, 1, 8, 2, p, null) == -1      # MTR_E_NULL
    assert hip_lib.mtr_se_gate(p, p, p, p, p, 2, 0, 1, 8, 2, null, null) == -1
    assert hip_lib.mtr_se_gate(p, p, p, p, p, 2, 0, 1, 6, 2, p, null) == -2         # C % 4 != 0
    assert hip_lib.mtr_se_gate(p, p, p, p, p, 2, 5, 1, 8, 2, p, null) == -4         # gate code
    assert hip_lib.mtr_se_gate(p, p, p, p, p, 9, 0, 1, 8, 2, p, null) == -4         # act code
    assert _lib.SIGNATURES['mtr_se_gate']


@pytest.mark.parametrize('name', ['efficientnetv2-s', 'mobilenetv3'])
def test_fused_se_forward_matches_the_unfused_folded_path(name, hip_lib):
    """The folded network with K12 against the same folded network with the squeeze-excite blocks on
    PyTorch's ops (mean_from cleared), batch 64 at 256 px: within 1e-4 relative (max-abs / max)."""
    import copy
    from metrabs_amd import backbones
    torch.manual_seed(0)
    net = backbones.calibrate_batchnorm(backbones.build_backbone(name).cuda(), 256, 'cuda', batch_size=4)
    fused = backbones.fold_batchnorm(net, fused_epilogue=True)
    plain = copy.deepcopy(fused)
    for m in plain.modules():
        if isinstance(m, backbones.SqueezeExcite):
            m.mean_from = ()
    x = torch.rand(64, 3, 256, 256, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    calls = []
    from metrabs_amd import kernels
    orig = kernels.se_gate

    def counting(*a, **k):
        calls.append(1)
        return orig(*a, **k)

    kernels.se_gate = counting
    try:
        with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
            a, b = plain(x), fused(x)
            b2 = fused(x)
    finally:
        kernels.se_gate = orig
    n_se = sum(isinstance(m, backbones.SqueezeExcite) for m in fused.modules())
    assert len(calls) == 2 * n_se > 0
    assert torch.equal(b, b2)
    assert float((a - b).abs().max()) <= 1e-4 * float(a.abs().max()), float((a - b).abs().max())


def test_fused_se_is_skipped_where_a_gradient_is_wanted(hip_lib):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    net = backbones.calibrate_batchnorm(backbones.build_backbone('mobilenetv3').cuda(), 128, 'cuda', batch_size=2)
    fused = backbones.fold_batchnorm(net, fused_epilogue=True)
    se = next(m for m in fused.modules() if isinstance(m, backbones.SqueezeExcite))
    assert not se._fused_gate_ok()      # parameters require grad, grad mode on
    with torch.no_grad():
        assert se._fused_gate_ok()

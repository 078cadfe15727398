"""GPU: K13, a 1x1 convolution as one f32 MFMA GEMM with the K10 epilogue and the squeeze-excite gate
folded in (csrc/conv1x1.hip), against an fp64 torch evaluation; its fallbacks; and the folded backbone
forward with it on against the same forward with it off."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ACTS = [None, 'relu', 'silu', 'hardswish']
_TORCH_ACT = {None: lambda t: t, 'relu': F.relu, 'silu': F.silu, 'hardswish': F.hardswish}


def _conv1x1_shapes(name, res=256):
    """(Cin, Cout, H, W, act, residual) of every 1x1 ConvBiasAct of a folded backbone at `res` px."""
    from metrabs_amd import backbones
    net = backbones.fold_batchnorm(backbones.build_backbone(name).eval(), fused_epilogue=True).cuda()
    shapes = set()

    def hook(mod, args, kwargs):
        x = args[0]
        if mod.conv.kernel_size == (1, 1) and mod.conv.stride == (1, 1):
            shapes.add((x.shape[1], mod.conv.out_channels, x.shape[2], x.shape[3], mod.act_name,
                        kwargs.get('residual') is not None))

    hs = [m.register_forward_pre_hook(hook, with_kwargs=True) for m in net.modules()
          if isinstance(m, backbones.ConvBiasAct)]
    with torch.inference_mode():
        net(torch.rand(1, 3, res, res, device='cuda'))
    for h in hs:
        h.remove()
    return sorted(shapes, key=str)


def _inputs(B, K, M, H, W, seed, gate, residual):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(B, K, H, W, device='cuda', generator=g)
    w = torch.randn(M, K, 1, 1, device='cuda', generator=g) / K ** 0.5
    b = 0.5 * torch.randn(M, device='cuda', generator=g)
    gt = torch.rand(B, K, device='cuda', generator=g) if gate else None
    r = torch.randn(B, M, H, W, device='cuda', generator=g) if residual else None
    return x, w, b, gt, r


def _reference(x, w, b, act, gt, r):
    """(fp64 result, bound): |got - fp64| <= a small multiple of 2^-23 * sum_k |w x| (the f32 MFMA is an fmaf chain),
    through the activation (Lipschitz <= 1.1 for every act here) plus its own f32 rounding."""
    xg = x if gt is None else x * gt[:, :, None, None]        # f32, rounded as torch's x * g
    wd = w.double().flatten(1)
    z = torch.einsum('mk,bkhw->bmhw', wd, xg.double()) + b.double()[None, :, None, None]
    s = torch.einsum('mk,bkhw->bmhw', wd.abs(), xg.double().abs()) + b.double().abs()[None, :, None, None]
    ref = _TORCH_ACT[act](z)
    if r is not None:
        ref = ref + r.double()
    return ref, 4 * 2.0 ** -23 * 1.1 * s + 1e-6 * ref.abs() + 1e-30


def _check(x, w, b, act, gt, r, got):
    """_reference's bound on every element (tests/conv_fuzz.py uses the same two functions)."""
    ref, bound = _reference(x, w, b, act, gt, r)
    assert got.shape == ref.shape and got.dtype == torch.float32
    excess = float(((got.double() - ref).abs() - bound).max())
    assert excess <= 0, excess


@pytest.mark.parametrize('name', ['efficientnetv2-s', 'efficientnetv2-l', 'mobilenetv3'])
@pytest.mark.parametrize('B', [1, 3, 64])
def test_conv1x1_matches_fp64_on_every_backbone_shape(name, B, hip_lib):
    """Every 1x1 shape of the backbone with its own activation and skip connection, with the gate on
    every other shape (the project convs take it in the network)."""
    from metrabs_amd import kernels
    shapes = _conv1x1_shapes(name)
    assert shapes
    for i, (K, M, H, W, act, res) in enumerate(shapes):
        if B == 64 and H * W > 64 * 64 and K * M > 64 * 64:
            continue   # (the first layers of MobileNetV3 at 128 px: covered at B = 1, 3)
        x, w, b, gt, r = _inputs(B, K, M, H, W, 1000 + i, gate=i % 2 == 0, residual=res)
        got = kernels.conv1x1_bias_act(x, w, b, act, gate=gt, residual=r)
        _check(x, w, b, act, gt, r, got)


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('gate', [False, True])
@pytest.mark.parametrize('residual', [False, True])
@pytest.mark.parametrize('shape', [(960, 160, 16, 16), (160, 960, 16, 16), (1536, 256, 8, 8), (64, 256, 32, 32),
                                   (24, 72, 12, 12), (200, 80, 4, 4)])
def test_conv1x1_every_epilogue(act, gate, residual, shape, hip_lib):
    from metrabs_amd import kernels
    K, M, H, W = shape
    x, w, b, gt, r = _inputs(3, K, M, H, W, 7, gate, residual)
    _check(x, w, b, act, gt, r, kernels.conv1x1_bias_act(x, w, b, act, gate=gt, residual=r))


def test_conv1x1_is_deterministic_and_graph_safe(hip_lib):
    from metrabs_amd import kernels
    x, w, b, gt, r = _inputs(64, 960, 160, 16, 16, 3, True, True)
    a = kernels.conv1x1_bias_act(x, w, b, None, gate=gt, residual=r)
    a2 = kernels.conv1x1_bias_act(x, w, b, None, gate=gt, residual=r)
    assert torch.equal(a, a2)
    with torch.inference_mode():
        out = torch.empty_like(a)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            kernels.conv1x1_bias_act(x, w, b, None, gate=gt, residual=r, out=out)
            st.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                kernels.conv1x1_bias_act(x, w, b, None, gate=gt, residual=r, out=out)
        torch.cuda.current_stream().wait_stream(st)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, a)


def _folded(name, res, batch_size=4):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    net = backbones.calibrate_batchnorm(backbones.build_backbone(name).cuda(), res, 'cuda', batch_size=batch_size)
    return net, backbones.fold_batchnorm(net, fused_epilogue=True)


def _paths(net):
    from metrabs_amd import backbones
    return [m.last_path for m in net.modules() if isinstance(m, backbones.ConvBiasAct)]


@pytest.mark.parametrize('name,res', [('efficientnetv2-s', 224), ('efficientnetv2-s', 160), ('mobilenetv3', 224),
                                      ('resnet18', 256)])
def test_conv1x1_falls_back_where_it_does_not_apply(name, res, hip_lib):
    """7x7 and 5x5 maps (H*W not a multiple of 4) and ResNet-18's stride-2 1x1 convolutions take the
    library path without raising, and give the unfolded network's function."""
    from metrabs_amd import backbones
    net, fused = _folded(name, res)
    x = torch.rand(2, 3, res, res, device='cuda')
    with torch.inference_mode():
        a, b = net(x), fused(x)
    assert float((a - b).abs().max()) <= 1e-3 * float(a.abs().max())
    paths = _paths(fused)
    assert 'library' in paths
    if name == 'resnet18':
        assert all(p == 'library' for p in paths)
    for m in fused.modules():
        if isinstance(m, backbones.ConvBiasAct) and m.last_path != 'library':
            assert m.conv.kernel_size == (1, 1) and m.conv.stride == (1, 1)


def test_conv1x1_falls_back_under_autocast_and_where_a_gradient_is_wanted(hip_lib):
    net, fused = _folded('mobilenetv3', 128, batch_size=2)
    x = torch.rand(2, 3, 128, 128, device='cuda')
    with torch.inference_mode(), torch.autocast('cuda', dtype=torch.float16):
        y16 = fused(x)
    assert y16.dtype == torch.float16 and set(_paths(fused)) == {'library'}
    y = fused(x)   # grad mode on, parameters require grad
    assert set(_paths(fused)) == {"library"}
    with torch.no_grad():
        fused(x)
    assert 'k13_gate' in _paths(fused)


@pytest.mark.parametrize('name', ['efficientnetv2-s', 'mobilenetv3'])
def test_folded_forward_with_k13_matches_it_off(name, hip_lib):
    """Batch 64 at 256 px: K13 on against K13 off (rocBLAS + K10 + x * gate), within 1e-4 relative
    (max-abs / max); every MBConv expand and project conv took K13, every project behind a
    squeeze-excite block with the gate folded in (no x * gate pass)."""
    from metrabs_amd import backbones
    _, fused = _folded(name, 256)
    x = torch.rand(64, 3, 256, 256, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    mbconv = (backbones.MBConv, backbones.MBv3Block)
    muls = []
    orig_mul = torch.Tensor.__mul__

    def counting_mul(a, b):
        if isinstance(b, torch.Tensor) and b.dim() == 4 and b.shape[2:] == (1, 1) and a.dim() == 4 \
                and a.shape[2:] != (1, 1):
            muls.append(tuple(a.shape))
        return orig_mul(a, b)

    try:
        backbones.ConvBiasAct.use_k13 = False
        with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
            a = fused(x)
        assert set(_paths(fused)) == {'library'}
        backbones.ConvBiasAct.use_k13 = True
        muls.clear()
        torch.Tensor.__mul__ = counting_mul
        with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
            b = fused(x)
        torch.Tensor.__mul__ = orig_mul
        with torch.inference_mode():
            b2 = fused(x)
    finally:
        torch.Tensor.__mul__ = orig_mul
        backbones.ConvBiasAct.use_k13 = True
    assert torch.equal(b, b2)
    assert float((a - b).abs().max()) <= 1e-4 * float(a.abs().max()), float((a - b).abs().max())
    n_blocks = n_gated = n_slower_gated = 0
    for blk in fused.modules():
        if not isinstance(blk, mbconv):
            continue
        layers = list(blk.block)
        for i, m in enumerate(layers):
            if isinstance(m, backbones.ConvBNAct) and isinstance(m[0], backbones.ConvBiasAct) and \
                    m[0].conv.kernel_size == (1, 1):
                n_blocks += 1
                gated = i > 0 and isinstance(layers[i - 1], backbones.SqueezeExcite)
                n_gated += gated
                c = m[0].conv
                if (c.in_channels, c.out_channels, 64) in backbones.ConvBiasAct.k13_slower and \
                        m[0].last_path == 'library':
                    n_slower_gated += gated   # (the dispatch table's measured losers: 8x8 maps)
                    continue
                assert m[0].last_path == ('k13_gate' if gated else 'k13'), (blk, i, m[0].last_path)
    assert n_blocks > 0 and n_gated > n_slower_gated
    assert len(muls) == n_slower_gated   # x * gate ran only in front of the library-path projects


def test_conv1x1_entry_point_argument_checks(hip_lib):
    """No GPU work: every call below is refused before a launch."""
    null = ctypes.c_void_p(0)
    t = torch.zeros(256, device='cuda')
    p = ctypes.c_void_p(t.data_ptr())
    q = ctypes.c_void_p(t.data_ptr() + 512)
    f = hip_lib.mtr_conv1x1_bias_act
    assert f(null, 0, p, p, null, null, 0, 1, 8, 8, 16, q, null) == -1     # MTR_E_NULL
    assert f(p, 0, p, p, null, null, 0, 1, 8, 8, 16, null, null) == -1
    assert f(p, 1, p, p, null, null, 0, 1, 8, 8, 16, q, null) == -3        # f16: the library path
    assert f(p, 0, p, p, null, null, 0, 1, 8, 8, 49, q, null) == -2        # H*W = 49
    assert f(p, 0, p, p, null, null, 0, 1, 8, 6, 16, q, null) == -2        # Cin = 6
    assert f(p, 0, p, p, null, null, 0, 1, 0, 8, 16, q, null) == -2
    assert f(p, 0, p, p, null, null, 7, 1, 8, 8, 16, q, null) == -4        # act code
    assert f(p, 0, p, p, null, null, 0, 1, 8, 8, 16, p, null) == -4        # y aliases x
    assert f(ctypes.c_void_p(t.data_ptr() + 4), 0, p, p, null, null, 0, 1, 8, 8, 16, q, null) == -6
    assert f(p, 0, p, p, null, null, 0, 0, 8, 8, 16, q, null) == 0         # B = 0: nothing to do

"""GPU: K13's forcible configurations (csrc/conv1x1.hip, mtr_conv1x1_bias_act_opts), the deep-K one above all: against
an fp64 torch evaluation, against each other bit for bit, guard bands, repeat calls, graph replay, base-pointer
alignment; and the folded EfficientNetV2-S forward with the shapes this kernel took off the library path."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ACTS = [None, 'relu', 'silu', 'hardswish']
_TORCH_ACT = {None: lambda t: t, 'relu': F.relu, 'silu': F.silu, 'hardswish': F.hardswish}
CONFIGS = ['wide', 'square', 'tall', 'deepk']
# (K, M, H, W).  The deep-K configuration stages k-tiles of 32 in a ring of three: 48 tiles; one partial tile (fewer
# tiles than stages); two tiles with a k tail of 4 and tiles spanning four images; M past one workgroup's 128 / 256
# channels with zero rows; four columns per image, 80 of 128 channels, a one-tile launch at B = 1; 16 tiles, the
# 4-column maps; exactly stages x BK = 96, and 96 + 4 (the guarded last steps with one k group in the fourth tile)
SHAPES = [(1536, 256, 8, 8), (8, 256, 8, 8), (36, 256, 4, 4), (96, 200, 8, 8), (100, 80, 2, 2), (512, 256, 4, 4),
          (96, 256, 8, 8), (100, 256, 8, 8)]


def _inputs(B, K, M, H, W, seed, gate, residual):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(B, K, H, W, device='cuda', generator=g)
    w = torch.randn(M, K, 1, 1, device='cuda', generator=g) / K ** 0.5
    b = 0.5 * torch.randn(M, device='cuda', generator=g)
    gt = torch.rand(B, K, device='cuda', generator=g) if gate else None
    r = torch.randn(B, M, H, W, device='cuda', generator=g) if residual else None
    return x, w, b, gt, r


def _check(x, w, b, act, gt, r, got):
    """The bound of tests/test_gpu_conv1x1.py::_check: |got - fp64| <= a small multiple of 2^-23 * sum_k |w x| (the f32
    MFMA is an fmaf chain), through the activation (Lipschitz <= 1.1 for every act here) plus its own f32 rounding."""
    xg = x if gt is None else x * gt[:, :, None, None]        # f32, rounded as torch's x * g
    wd = w.double().flatten(1)
    z = torch.einsum('mk,bkhw->bmhw', wd, xg.double()) + b.double()[None, :, None, None]
    s = torch.einsum('mk,bkhw->bmhw', wd.abs(), xg.double().abs()) + b.double().abs()[None, :, None, None]
    ref = _TORCH_ACT[act](z)
    if r is not None:
        ref = ref + r.double()
    bound = 4 * 2.0 ** -23 * 1.1 * s + 1e-6 * ref.abs() + 1e-30
    assert got.shape == ref.shape and got.dtype == torch.float32
    excess = float(((got.double() - ref).abs() - bound).max())
    assert excess <= 0, excess


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('gate', [False, True])
@pytest.mark.parametrize('residual', [False, True])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_every_configuration_matches_fp64_and_every_other(shape, B, residual, gate, act, hip_lib):
    from metrabs_amd import kernels
    K, M, H, W = shape
    x, w, b, gt, r = _inputs(B, K, M, H, W, 17 + B, gate, residual)
    G = 256   # floats: the guarded output stays 16-byte aligned
    n = B * M * H * W
    big = torch.full((n + 2 * G,), -7.0, device='cuda')
    out = big[G:G + n].view(B, M, H, W)
    first = None
    for config in CONFIGS:
        assert kernels.conv1x1_plan(M, K, H * W, B, config)[0] == config
        out.fill_(-7.0)
        got = kernels.conv1x1_bias_act(x, w, b, act, gate=gt, residual=r, out=out, config=config)
        torch.cuda.synchronize()
        assert got is out
        assert bool((big[:G] == -7.0).all()) and bool((big[G + n:] == -7.0).all()), config
        if first is None:
            _check(x, w, b, act, gt, r, out)
            first = out.clone()
        else:
            assert torch.equal(out, first), config   # the bits do not depend on the tile
    assert torch.equal(kernels.conv1x1_bias_act(x, w, b, act, gate=gt, residual=r), first)


@pytest.mark.parametrize('config', CONFIGS)
@pytest.mark.parametrize('shape', [(1536, 256, 8, 8), (100, 80, 2, 2)])
def test_forced_configuration_repeats_itself_and_replays(shape, config, hip_lib):
    from metrabs_amd import kernels
    K, M, H, W = shape
    x, w, b, gt, r = _inputs(3, K, M, H, W, 3, True, True)
    a = kernels.conv1x1_bias_act(x, w, b, 'silu', gate=gt, residual=r, config=config)
    a2 = kernels.conv1x1_bias_act(x, w, b, 'silu', gate=gt, residual=r, config=config)
    assert torch.equal(a, a2)
    with torch.inference_mode():
        out = torch.empty_like(a)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            kernels.conv1x1_bias_act(x, w, b, 'silu', gate=gt, residual=r, out=out, config=config)
            st.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                kernels.conv1x1_bias_act(x, w, b, 'silu', gate=gt, residual=r, out=out, config=config)
        torch.cuda.current_stream().wait_stream(st)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, a)


@pytest.mark.parametrize('config', CONFIGS)
def test_shifted_aligned_base_is_accepted_and_unaligned_refused(config, hip_lib):
    from metrabs_amd import kernels
    B, K, M, H, W = 3, 100, 80, 2, 2
    x, w, b, gt, r = _inputs(B, K, M, H, W, 9, True, True)
    ref = kernels.conv1x1_bias_act(x, w, b, 'relu', gate=gt, residual=r, config=config)

    def shifted(t, floats):
        big = torch.zeros(t.numel() + 8, device='cuda')
        v = big[floats:floats + t.numel()].view(t.shape)
        v.copy_(t)
        return v

    xs, ws, rs = shifted(x, 4), shifted(w, 4), shifted(r, 4)    # 16 bytes past the allocation's base
    out = shifted(torch.zeros_like(ref), 4)
    assert xs.data_ptr() % 16 == 0 and xs.data_ptr() % 32 != 0
    kernels.conv1x1_bias_act(xs, ws, b, 'relu', gate=gt, residual=rs, out=out, config=config)
    assert torch.equal(out, ref)
    code = kernels.CONV1X1_CONFIGS[config]
    null = ctypes.c_void_p(0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    f = hip_lib.mtr_conv1x1_bias_act_opts
    args = lambda xx, ww, rr, yy: (p(xx), 0, p(ww), p(b), p(gt), p(rr), 1, B, M, K, H * W, p(yy), null, code)
    for bad in (shifted(x, 1), shifted(x, 2)):                  # 4 and 8 bytes off
        assert f(*args(bad, w, r, out)) == -6                   # MTR_E_ALIGN
    assert f(*args(x, shifted(w, 1), r, out)) == -6
    assert f(*args(x, w, shifted(r, 3), out)) == -6
    assert f(*args(x, w, r, shifted(ref, 1))) == -6


def test_opts_and_plan_argument_checks(hip_lib):
    """No GPU work: every call below is refused before a launch (or is host only)."""
    from metrabs_amd import _lib, kernels
    null = ctypes.c_void_p(0)
    t = torch.zeros(256, device='cuda')
    p = ctypes.c_void_p(t.data_ptr())
    q = ctypes.c_void_p(t.data_ptr() + 512)
    f = hip_lib.mtr_conv1x1_bias_act_opts
    assert _lib.SIGNATURES['mtr_conv1x1_bias_act_opts'] and _lib.SIGNATURES['mtr_conv1x1_plan']
    for config in (-1, 0, 1, 2, 3):
        assert f(null, 0, p, p, null, null, 0, 1, 8, 8, 16, q, null, config) == -1     # MTR_E_NULL
        assert f(p, 1, p, p, null, null, 0, 1, 8, 8, 16, q, null, config) == -3        # f16: the library path
        assert f(p, 0, p, p, null, null, 0, 1, 8, 8, 49, q, null, config) == -2        # H*W = 49
        assert f(p, 0, p, p, null, null, 0, 1, 8, 6, 16, q, null, config) == -2        # Cin = 6
        assert f(p, 0, p, p, null, null, 7, 1, 8, 8, 16, q, null, config) == -4        # act code
        assert f(p, 0, p, p, null, null, 0, 1, 8, 8, 16, p, null, config) == -4        # y aliases x
        assert f(p, 0, p, p, null, null, 0, 0, 8, 8, 16, q, null, config) == 0         # B = 0: nothing to do
    assert f(p, 0, p, p, null, null, 0, 1, 8, 8, 16, q, null, 4) == -4                 # no such configuration
    assert f(p, 0, p, p, null, null, 0, 1, 8, 8, 16, q, null, -2) == -4
    plan = (ctypes.c_int * 4)()
    g = hip_lib.mtr_conv1x1_plan
    assert g(256, 1536, 64, 64, 3, null) == -1
    assert g(0, 1536, 64, 64, 3, ctypes.addressof(plan)) == -2
    assert g(256, 1536, 64, 64, 9, ctypes.addressof(plan)) == -4
    assert g(256, 1536, 64, 64, 3, ctypes.addressof(plan)) == 0 and list(plan) == [3, 8, 256, 16]
    assert kernels.conv1x1_plan(128, 512, 256, 64, 'deepk') == ('deepk', 4, 128, 16)
    assert kernels.conv1x1_plan(200, 96, 64, 3, 'tall') == ('tall', 4, 128, 32)
    # the library's own choice is a function of the shape alone
    assert kernels.conv1x1_plan(256, 1536, 64, 64) == kernels.conv1x1_plan(256, 1536, 64, 64, 'auto')


def test_shapes_taken_off_the_library_path_run_on_k13(hip_lib):
    """Folded EfficientNetV2-S at 256 px, batch 2: 960 -> 256 (the first stage-6 project) and the 256 -> 1280 head left
    k13_slower; every gated project whose shape is not in it reports 'k13_gate', x * gate passes run only in front of
    the ones that are, and the output is within 1e-4 relative (max-abs over max) of the same forward with K13 off."""
    from metrabs_amd import backbones
    torch.manual_seed(0)
    net = backbones.calibrate_batchnorm(backbones.build_backbone('efficientnetv2-s').cuda(), 256, 'cuda', batch_size=4)
    fused = backbones.fold_batchnorm(net, fused_epilogue=True)
    x = torch.rand(2, 3, 256, 256, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
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
        backbones.ConvBiasAct.use_k13 = True
        torch.Tensor.__mul__ = counting_mul
        with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
            b = fused(x)
    finally:
        torch.Tensor.__mul__ = orig_mul
        backbones.ConvBiasAct.use_k13 = True
    assert float((a - b).abs().max()) <= 1e-4 * float(a.abs().max()), float((a - b).abs().max())
    slower = backbones.ConvBiasAct.k13_slower
    assert (960, 256, 64) not in slower and (256, 1280, 64) not in slower   # the shapes this change moved
    seen = {}
    n_library = 0
    for blk in fused.modules():
        if not isinstance(blk, backbones.MBConv):
            continue
        layers = list(blk.block)
        for i, m in enumerate(layers):
            if i > 0 and isinstance(layers[i - 1], backbones.SqueezeExcite) and isinstance(m, backbones.ConvBNAct) \
                    and isinstance(m[0], backbones.ConvBiasAct):
                c = m[0].conv
                if (c.in_channels, c.out_channels, 64) in slower:
                    assert m[0].last_path == 'library'
                    n_library += 1
                    continue
                assert m[0].last_path == 'k13_gate', (c.in_channels, c.out_channels, m[0].last_path)
                seen[(c.in_channels, c.out_channels)] = seen.get((c.in_channels, c.out_channels), 0) + 1
    assert seen.get((960, 256)) == 1
    assert len(muls) == n_library
    heads = [m for m in fused.modules() if isinstance(m, backbones.ConvBiasAct) and m.conv.in_channels == 256
             and m.conv.out_channels == 1280]
    assert len(heads) == 1 and heads[0].last_path == 'k13'

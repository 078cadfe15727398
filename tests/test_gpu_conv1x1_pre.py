"""GPU: K13's input prologue (csrc/conv1x1.hip, mtr_conv1x1_bias_act_pre) -- the "+ bias, activation" of the
convolution in front applied to every element on its way into the GEMM -- against K10 followed by K13 bit for bit,
in every configuration; against fp64; guard bands, repeats, graph replay, argument checks; and the f32 folded
EfficientNetV2 copies whose FusedMBConv blocks use it (backbones.FusedMBConv.pre_pair)."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ACTS = [None, 'relu', 'silu', 'hardswish']
_TORCH_ACT = {None: lambda t: t, 'relu': F.relu, 'silu': F.silu, 'hardswish': F.hardswish}
# (K, M, H, W): a k tail under BK 16, columns past B * HW at B = 1, M under one tile; a k tail under BK 32, tiles
# spanning images; two project classes of EfficientNetV2-S on small maps; M past two tiles; fewer k-tiles than ring
# stages; deep-K with a tail; and three 32-channel tiles whose weight still fits the streaming configuration's LDS
SHAPES = [(20, 24, 4, 4), (36, 48, 4, 4), (96, 48, 8, 8), (192, 72, 4, 8), (256, 64, 8, 8), (12, 160, 4, 4),
          (260, 256, 4, 4), (68, 72, 4, 4)]


def _configs():
    from metrabs_amd import kernels
    return [c for c in kernels.CONV1X1_CONFIGS if c != 'auto'] + ['auto']


def _inputs(B, K, M, H, W, seed, gate, residual):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(B, K, H, W, device='cuda', generator=g)
    w = torch.randn(M, K, 1, 1, device='cuda', generator=g) / K ** 0.5
    b = 0.5 * torch.randn(M, device='cuda', generator=g)
    # around +3: act(b_in) is far from zero, so an entry that should be a zero fill and got the prologue shows up
    b_in = 3.0 + 0.5 * torch.randn(K, device='cuda', generator=g)
    gt = torch.rand(B, K, device='cuda', generator=g) if gate else None
    r = torch.randn(B, M, H, W, device='cuda', generator=g) if residual else None
    return x, w, b, b_in, gt, r


def _check(x, w, b, act, gt, r, got):
    """The bound of tests/test_gpu_conv1x1.py::_check on the GEMM input `x` (here: K10's output, itself held to fp64 by
    tests/test_gpu_bias_act.py): |got - fp64| <= a small multiple of 2^-23 * sum_k |w x| (the f32 MFMA is an fmaf
    chain), through the activation (Lipschitz <= 1.1 for every act here) plus its own f32 rounding."""
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


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_prologue_has_the_bits_of_k10_then_k13_in_every_configuration(shape, B, hip_lib):
    from metrabs_amd import kernels
    K, M, H, W = shape
    G = 256   # floats: the guarded output stays 16-byte aligned
    n = B * M * H * W
    big = torch.full((n + 2 * G,), -7.0, device='cuda')
    out = big[G:G + n].view(B, M, H, W)
    for gate, residual in itertools.product([False, True], repeat=2):
        x, w, b, b_in, gt, r = _inputs(B, K, M, H, W, 31 + B, gate, residual)
        x_kept = x.clone()
        for a_in in ACTS:
            x10 = kernels.bias_act_(x.clone(), b_in, a_in)     # what K10 leaves in the tensor
            for act in (None, 'silu'):
                what = (gate, residual, a_in, act)
                want = kernels.conv1x1_bias_act(x10, w, b, act, gate=gt, residual=r)
                _check(x10, w, b, act, gt, r, want)
                for config in _configs():
                    out.fill_(-7.0)
                    got = kernels.conv1x1_bias_act(x, w, b, act, gate=gt, residual=r, out=out, config=config,
                                                   in_bias=b_in, in_act=a_in)
                    assert got is out
                    assert torch.equal(out, want), (what, config)
                    assert bool((big[:G] == -7.0).all()) and bool((big[G + n:] == -7.0).all()), (what, config)
        assert torch.equal(x, x_kept)   # the prologue reads x, it does not finish it in place


@pytest.mark.parametrize('shape', [(192, 48, 8, 8), (36, 48, 4, 4), (260, 256, 4, 4)])
def test_prologue_repeats_itself_and_replays(shape, hip_lib):
    from metrabs_amd import kernels
    K, M, H, W = shape
    x, w, b, b_in, gt, r = _inputs(3, K, M, H, W, 5, True, True)
    for config in _configs():
        kw = dict(gate=gt, residual=r, config=config, in_bias=b_in, in_act='silu')
        a = kernels.conv1x1_bias_act(x, w, b, None, **kw)
        assert torch.equal(a, kernels.conv1x1_bias_act(x, w, b, None, **kw))
        with torch.inference_mode():
            out = torch.empty_like(a)
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                kernels.conv1x1_bias_act(x, w, b, None, out=out, **kw)
                st.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                    kernels.conv1x1_bias_act(x, w, b, None, out=out, **kw)
            torch.cuda.current_stream().wait_stream(st)
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, a), config


def test_pre_entry_argument_checks(hip_lib):
    """No GPU work: every call below is refused before a launch (or is host only)."""
    from metrabs_amd import _lib, kernels
    null = ctypes.c_void_p(0)
    t = torch.zeros(256, device='cuda')
    p = ctypes.c_void_p(t.data_ptr())
    q = ctypes.c_void_p(t.data_ptr() + 512)
    odd = ctypes.c_void_p(t.data_ptr() + 2)
    f = hip_lib.mtr_conv1x1_bias_act_pre
    assert _lib.SIGNATURES['mtr_conv1x1_bias_act_pre']
    #        x  dtype w  bias in_bias in_act gate residual act B  M  K  HW  y  stream config
    assert f(null, 0, p, p, p, 2, null, null, 0, 1, 8, 8, 16, q, null, -1) == -1      # MTR_E_NULL
    assert f(p, 1, p, p, p, 2, null, null, 0, 1, 8, 8, 16, q, null, -1) == -3         # f16: the library path
    assert f(p, 0, p, p, p, 2, null, null, 0, 1, 8, 8, 49, q, null, -1) == -2         # H*W = 49
    assert f(p, 0, p, p, null, 2, null, null, 0, 1, 8, 8, 16, q, null, -1) == -4      # in_act without in_bias
    assert f(p, 0, p, p, p, 7, null, null, 0, 1, 8, 8, 16, q, null, -1) == -4         # in_act code
    assert f(p, 0, p, p, p, -1, null, null, 0, 1, 8, 8, 16, q, null, -1) == -4
    assert f(p, 0, p, p, odd, 2, null, null, 0, 1, 8, 8, 16, q, null, -1) == -6       # MTR_E_ALIGN
    assert f(p, 0, p, p, p, 2, null, null, 0, 1, 8, 8, 16, p, null, -1) == -4         # y aliases x
    assert f(p, 0, p, p, p, 2, null, null, 0, 0, 8, 8, 16, q, null, -1) == 0          # B = 0: nothing to do
    assert f(p, 0, p, p, null, 0, null, null, 0, 0, 8, 8, 16, q, null, -1) == 0
    assert f(p, 0, p, p, p, 2, null, null, 0, 1, 8, 8, 16, q, null, 9) == -4          # no such configuration
    # the entry from before the prologue keeps its range of configurations
    assert hip_lib.mtr_conv1x1_bias_act_opts(p, 0, p, p, null, null, 0, 1, 8, 8, 16, q, null, 4) == -4
    # the streaming configuration: through this entry and the plan only; 'tall' where the weight does not fit LDS
    assert f(p, 0, p, p, p, 2, null, null, 0, 0, 8, 8, 16, q, null, 4) == 0
    plan = (ctypes.c_int * 4)()
    g = hip_lib.mtr_conv1x1_plan
    assert g(48, 192, 4096, 64, 4, ctypes.addressof(plan)) == 0 and list(plan) == [4, 2, 64, 256]
    assert g(64, 256, 1024, 64, 4, ctypes.addressof(plan)) == 0 and list(plan) == [4, 2, 64, 128]
    assert g(72, 192, 32, 3, 4, ctypes.addressof(plan)) == 0 and list(plan) == [2, 3, 96, 32]
    assert kernels.conv1x1_plan(72, 68, 16, 3, 'stream') == ('stream', 3, 96, 128)
    assert kernels.conv1x1_plan(256, 260, 16, 3, 'stream')[0] == 'tall'
    x = torch.zeros(1, 8, 4, 4, device='cuda')
    w = torch.zeros(8, 8, device='cuda')
    with pytest.raises(ValueError):
        kernels.conv1x1_bias_act(x, w, w[0], None, in_act='silu')
    with pytest.raises(ValueError):
        kernels.conv1x1_bias_act(x, w, w[0], None, in_bias=torch.zeros(4, device='cuda'), in_act='silu')


# ---- the network

def _copy(name, res):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    net = backbones.calibrate_batchnorm(backbones.build_backbone(name).cuda(), res, 'cuda', batch_size=2)
    return backbones.fold_batchnorm(net, fused_epilogue=True)


def _run(copy, x, switch):
    from metrabs_amd import backbones, kernels
    FM = backbones.FusedMBConv
    calls = []
    orig = kernels.bias_act_

    def counting(y, *a, **k):
        calls.append(tuple(y.shape))
        return orig(y, *a, **k)

    try:
        FM.use_k13_pre = switch
        kernels.bias_act_ = counting
        with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, deterministic=True, benchmark=False):
            y = copy(x).clone()
    finally:
        FM.use_k13_pre = True
        kernels.bias_act_ = orig
    return y, calls


@pytest.mark.parametrize('name', ['efficientnetv2-s', 'efficientnetv2-l'])
def test_armed_copy_equals_the_chain_and_skips_k10(name, hip_lib):
    from metrabs_amd import backbones
    FM = backbones.FusedMBConv
    copy = _copy(name, 64)
    armed = [m for m in copy.modules() if isinstance(m, FM) and m.pre_pair]
    assert armed and len(armed) == (8 if name.endswith('-s') else 14)
    x = torch.rand(2, 3, 64, 64, device='cuda', generator=torch.Generator(device='cuda').manual_seed(4))

    heights = {}
    hs = [m.register_forward_pre_hook(lambda mod, args: heights.__setitem__(mod, args[0].shape[2])) for m in armed]
    off, calls_off = _run(copy, x, False)
    for h in hs:
        h.remove()
    assert all(m.last_path == 'chain' for m in armed)
    assert all(m.pre_pair[0].last_path == 'library' and m.pre_pair[1].last_path == 'k13' for m in armed)
    on, calls_on = _run(copy, x, True)
    assert torch.equal(on, off)
    skipped = []   # the tensors K10 is not called for: the expanded activations of the deferred blocks
    for m in armed:
        first, project = m.pre_pair
        c, h = first.conv, heights[m]
        assert first.last_path == 'library' and project.last_path == 'k13'
        slower = (c.in_channels, c.out_channels, project.conv.out_channels, c.stride[0], h, h) in FM.k13_pre_slower
        assert m.last_path == ('chain' if slower else 'k13_pre'), m.last_path
        if not slower:
            ho = (h - 1) // c.stride[0] + 1
            skipped.append((2, c.out_channels, ho, ho))
    assert skipped
    rest = list(calls_off)
    for c in calls_on:
        rest.remove(c)
    assert sorted(rest) == sorted(skipped)
    # the same tree and keys: nothing is registered twice
    sd = copy.state_dict()
    assert len(sd) == len(list(copy.named_parameters())) + len(list(copy.named_buffers()))
    assert not any('pre_pair' in k for k in sd)
    assert {'1.2.0.block.0.0.conv.weight', '1.2.0.block.0.0.bias', '1.2.0.block.1.0.conv.weight',
            '1.2.0.block.1.0.bias'} <= set(sd)


def test_armed_copy_on_odd_maps_takes_the_chain(hip_lib):
    """100 px: 25 x 25 and 13 x 13 maps in stages 2 and 3 (H * W not a multiple of 4): K13 does not take them, the
    block finishes the 3x3 layer as an unarmed one does."""
    from metrabs_amd import backbones
    FM = backbones.FusedMBConv
    copy = _copy('efficientnetv2-s', 100)
    armed = [m for m in copy.modules() if isinstance(m, FM) and m.pre_pair]
    x = torch.rand(2, 3, 100, 100, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5))
    on, calls_on = _run(copy, x, True)
    assert all(m.last_path == 'chain' for m in armed)
    assert all(m.pre_pair[0].last_path == 'library' and m.pre_pair[1].last_path == 'library' for m in armed)
    off, calls_off = _run(copy, x, False)
    assert torch.equal(on, off) and calls_on == calls_off
    try:
        for m in armed:
            m.pre_pair = ()   # (an instance attribute over the armed one: the block as it was before)
        assert not any(m.pre_pair for m in copy.modules() if isinstance(m, FM))
        plain, _ = _run(copy, x, True)
    finally:
        for m in armed:
            del m.pre_pair
    assert torch.equal(on, plain)

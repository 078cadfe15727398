"""GPU: K26h (csrc/expand_dw16_planes.hip), K25h's function -- the 1x1 expand of an MBConv block of the 16-bit
inference copy (K13h) and the stride-1 depthwise 3x3 layer behind it as one launch with the expanded activation in
LDS -- on the planes K11 runs on its GENERIC kernel (24x24 and 12x12 of a 384 px input).

Three independent checks per shape.  (a) BITS: y and the mean torch.equal to kernels.conv1x1_bias_act16 followed by
kernels.depthwise3x3_bias_act(.., 1, 1, want_mean=True) on the same tensors -- the kernel's contract -- and to
conv1x1_bias_act16 followed by kernels.depthwise3x3_blocks_bias_act (K18), which has the generic kernel's bits too.
(b) fp64, independently of the chain: the two layers in float64 on the 16-bit operands, the intermediate NOT rounded.
(c) small integers, exact.

The fp64 bound is the one of tests/test_gpu_expand_dw16.py, restated (its code is imported from there; it was written
down before K26h first ran and has not changed).  u = 2^-24, u_out = one rounding of the 16-bit format (2^-11 f16,
2^-8 bf16), ulp(v) = one unit in the last place of the format at |v|, L(act) the activation's Lipschitz constant (1 none
and relu, 1.1 silu, 1.5 hardswish).  With z1 = W1 x + b1, s1 = |W1| |x| + |b1|, m = act1(z1):

    d_mid = ulp(m) + L(act1) * Cin * u * s1 + 1e-6 |m| + u

With v = b2 + sum Wd m (fp64, m unrounded), c = sum |Wd| d_mid, S = sum |Wd| (|m| + d_mid) + |b2| and ref = act2(v):

    E     = 1.5 * 11 u S + (8 + 2 (|v| + c)) u (|ref| + L(act2) c)
            (K11's own bound of test_gpu_depthwise3x3.py: nine fma AND the bias -- eleven operations whatever their
            order, so the generic kernel's "accumulator from 0, bias last" is covered as the block kernel's "bias first"
            is -- through an activation evaluated in f32)
    bound = (L(act2) c + E) (1 + u_out) + u_out |ref| + tiny          (tiny = 2^-25 f16, 2^-126 bf16)

The mean: |mean_hat - mean(y)| <= (H W + 1) u mean |y| + 2^-126 (the f32 sum of the H W stored outputs in any order,
times the rounded 1 / (H W)).

Every element is checked; the largest error as a share of the bound is printed (DESIGN.md section 31 records it).
Then: every activation pair, determinism, both mappings, out=, graph replay, guard bands, the wrapper's refusals; the
armed copies of EfficientNetV2-S at 384 px and 256 px (paths, switches, the other options, K25h's among them); the
loader and the API on a 384 px model."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cases
from test_gpu_expand_dw16 import ACTS, DTYPES, _act64, _calibrated, _chain, _check_fp64, _inputs, _paths, _poses

pytestmark = pytest.mark.gpu

# (Cin, Cmid, H, W): the smallest shapes at which each mechanism can go wrong
SHAPES = [
    (40, 136, 12, 12),    # half a k step; a chunk tail of 8 at CM = 128; a half-dead position tile; one mean chunk
    (24, 72, 24, 24),     # three mean chunks with uneven lanes; a partial chunk at CM = 64
    (16, 32, 20, 20),     # two mean chunks; 12.5 tiles
    (8, 16, 6, 8),        # H % 4 != 0; lpp = 16
    (8, 8, 2, 4),         # lpp = 2; one partial tile
    (8, 16, 10, 4),       # rectangular planes: a transposed index shows
    (24, 96, 12, 24),
    (24, 96, 24, 12),
]
NETWORK_SHAPES = [(384, 2304, 12, 12), (224, 1344, 24, 24)]   # EfficientNetV2-L's own classes, B = 1


def _k18_chain(x, w1, b1, act1, wd, b2, act2):
    from metrabs_amd import kernels
    mid = kernels.conv1x1_bias_act16(x, w1, b1, act1)
    return kernels.depthwise3x3_blocks_bias_act(mid, wd, b2, act2, want_mean=True)


def _bits_and_bound(shape, B, dtype):
    from metrabs_amd import kernels
    Cin, Cmid, H, W = shape
    x, w1, b1, wd, b2 = _inputs(B, Cin, Cmid, H, W, 100 + Cin + H, dtype)
    assert kernels.expand_depthwise16_planes_supported(x, w1), shape
    assert not kernels.expand_depthwise16_supported(x, w1)
    assert kernels.conv1x1_16_supported(x, w1) and not kernels.k11_takes_block_kernel(H, W)
    got, mean = kernels.expand_depthwise16_planes(x, w1, b1, 'silu', wd, b2, 'silu', want_mean=True)
    for name, (want, wmean) in (('k11', _chain(x, w1, b1, 'silu', wd, b2, 'silu')),
                                ('k18', _k18_chain(x, w1, b1, 'silu', wd, b2, 'silu'))):
        diff = (got.float() - want.float()).abs()
        assert torch.equal(got, want), (name, shape, int((got != want).sum()), float(diff.max()))
        assert torch.equal(mean, wmean), (name, shape, int((mean != wmean).sum()))
    _check_fp64(x, w1, b1, 'silu', wd, b2, 'silu', got, mean, f'k26h {shape} B={B}')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_k26h_has_the_chains_bits_and_meets_the_fp64_bound(shape, B, dtype, hip_lib):
    _bits_and_bound(shape, B, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', NETWORK_SHAPES)
def test_k26h_on_the_networks_own_classes(shape, dtype, hip_lib):
    _bits_and_bound(shape, 1, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('act2', ACTS)
@pytest.mark.parametrize('act1', ACTS)
def test_k26h_every_activation_pair_with_and_without_the_mean(act1, act2, dtype, hip_lib):
    from metrabs_amd import kernels
    x, w1, b1, wd, b2 = _inputs(3, 40, 136, 12, 12, 11, dtype)
    want, wmean = _chain(x, w1, b1, act1, wd, b2, act2)
    got, mean = kernels.expand_depthwise16_planes(x, w1, b1, act1, wd, b2, act2, want_mean=True)
    assert torch.equal(got, want) and torch.equal(mean, wmean)
    _check_fp64(x, w1, b1, act1, wd, b2, act2, got, mean, f'k26h 40-136 12x12 {act1}/{act2}')
    alone = kernels.expand_depthwise16_planes(x, w1, b1, act1, wd, b2, act2)
    assert isinstance(alone, torch.Tensor) and torch.equal(alone, want)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('act', [None, 'relu'])
@pytest.mark.parametrize('shape', [(24, 200, 12, 12), (24, 72, 24, 24)])
def test_k26h_is_exact_on_small_integers(shape, act, dtype, hip_lib):
    """Small-integer data, an expand that looks at two input channels per output channel and an asymmetric depthwise
    weight (every tap distinct): every product, every partial sum, the intermediate and the output are integers of at
    most 2^8 in magnitude (exact in bf16, hence in f16), checked here on the reference -- so the result must EQUAL
    the integer evaluation: a swapped tap, a transposed fragment, a wrong tile, chunk or halo cannot hide in rounding.
    Both shapes are two chunks of channels, the last one partial."""
    from metrabs_amd import kernels
    Cin, Cmid, H, W = shape
    g = torch.Generator(device='cuda').manual_seed(3)
    x = torch.randint(-1, 2, (2, Cin, H, W), device='cuda', generator=g).float()
    c = torch.arange(Cmid, device='cuda')
    w1 = torch.zeros(Cmid, Cin, device='cuda')
    w1[c, c % Cin] = torch.where(c % 2 == 0, 1.0, -1.0)
    w1[c, (5 * c + 7) % Cin] += torch.where(c % 3 == 0, 2.0, -1.0)
    b1 = c.float() % 3 - 1
    taps = torch.tensor([1.0, -2.0, 3.0, -1.0, 2.0, -3.0, 2.0, 1.0, -1.0], device='cuda')
    wd = torch.stack([torch.roll(taps, int(i)) for i in range(9)])[c % 9].view(Cmid, 1, 3, 3) \
        * torch.where(c % 2 == 0, 1.0, -1.0).view(-1, 1, 1, 1)
    b2 = c.float() % 7 - 3
    mid = _act64(F.conv2d(x.double(), w1.double()[:, :, None, None], b1.double()), act)
    ref = _act64(F.conv2d(mid, wd.double(), b2.double(), 1, 1, groups=Cmid), act)
    limit = 2 ** 8
    assert float(mid.abs().max()) <= 5 and float(ref.abs().max()) <= 16 * 5 + 3 <= limit
    assert float(ref.abs().max()) > 20   # (not a trivially small case)
    got, mean = kernels.expand_depthwise16_planes(x.to(dtype), w1.to(dtype), b1, act, wd, b2, act, want_mean=True)
    assert torch.equal(got.double(), ref)
    # at most 576 integers of at most 2^7: every partial sum is exact in f32, in any order; then ONE f32 product with
    # the rounded 1 / (H W)
    inv = torch.tensor(1.0, device='cuda') / torch.tensor(float(H * W), device='cuda')
    assert torch.equal(mean, ref.sum((2, 3)).float() * inv)


@pytest.mark.parametrize('dtype', DTYPES)
def test_k26h_is_deterministic_graph_safe_and_stays_inside_y_and_the_mean(dtype, hip_lib):
    from metrabs_amd import kernels
    fn = kernels.expand_depthwise16_planes
    # B = 9: with the XCD mapping the grid is padded to 16 images, and workgroups past the batch leave at once
    for (B, Cin, Cmid, H, W) in [(9, 40, 136, 12, 12), (2, 24, 72, 24, 24)]:
        x, w1, b1, wd, b2 = _inputs(B, Cin, Cmid, H, W, 5, dtype)
        a, am = fn(x, w1, b1, 'silu', wd, b2, 'silu', want_mean=True)
        a2, am2 = fn(x, w1, b1, 'silu', wd, b2, 'silu', want_mean=True)
        assert torch.equal(a, a2) and torch.equal(am, am2)
        want, wmean = _chain(x, w1, b1, 'silu', wd, b2, 'silu')
        assert torch.equal(a, want) and torch.equal(am, wmean)
        for mapping in ('plain', 'xcd'):   # the bits do not depend on where a workgroup runs
            o, m = fn(x, w1, b1, 'silu', wd, b2, 'silu', want_mean=True, mapping=mapping)
            assert torch.equal(o, a) and torch.equal(m, am)
        # out= inside guard bands (64 elements either side: y's base stays 16-byte aligned)
        flat = torch.full((a.numel() + 128,), 7.0, device='cuda', dtype=dtype)
        out = flat[64:64 + a.numel()].view_as(a)
        assert fn(x, w1, b1, 'silu', wd, b2, 'silu', out=out) is out
        assert torch.equal(out, a)
        assert bool((flat[:64] == 7.0).all()) and bool((flat[-64:] == 7.0).all())
        # the mean inside guard bands, through the C entry, with both mappings
        wdf = wd.contiguous().float()
        for mapping in (0, 1):
            mflat = torch.full((am.numel() + 128,), 7.0, device='cuda')
            out.zero_()
            rc = hip_lib.mtr_expand_dw16_planes_opts(
                ctypes.c_void_p(x.data_ptr()), 1 if dtype == torch.float16 else 2, ctypes.c_void_p(w1.data_ptr()),
                ctypes.c_void_p(b1.data_ptr()), 2, ctypes.c_void_p(wdf.data_ptr()), ctypes.c_void_p(b2.data_ptr()), 2,
                B, Cin, Cmid, H, W, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(mflat.data_ptr() + 64 * 4),
                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), mapping)
            assert rc == 0
            torch.cuda.synchronize()
            assert torch.equal(mflat[64:-64].view_as(am), am) and torch.equal(out, a)
            assert bool((mflat[:64] == 7.0).all()) and bool((mflat[-64:] == 7.0).all())
            assert bool((flat[:64] == 7.0).all()) and bool((flat[-64:] == 7.0).all())
        with torch.inference_mode():
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                fn(x, w1, b1, 'silu', wd, b2, 'silu', out=out)
                st.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                    fn(x, w1, b1, 'silu', wd, b2, 'silu', out=out)
            torch.cuda.current_stream().wait_stream(st)
            for _ in range(2):
                out.zero_()
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, a)
            assert bool((flat[:64] == 7.0).all()) and bool((flat[-64:] == 7.0).all())
        # a shifted, 16-byte-aligned base of x is accepted, one 8 bytes off is refused
        xflat = torch.zeros(x.numel() + 8, device='cuda', dtype=dtype)
        x8 = xflat[8:].view_as(x).copy_(x)
        assert kernels.expand_depthwise16_planes_supported(x8, w1)
        assert torch.equal(fn(x8, w1, b1, 'silu', wd, b2, 'silu'), a)
        x4 = xflat[4:4 + x.numel()].view_as(x)
        assert not kernels.expand_depthwise16_planes_supported(x4, w1)
        with pytest.raises(RuntimeError):
            fn(x4, w1, b1, 'silu', wd, b2, 'silu')


def test_k26h_wrapper_argument_checks(hip_lib):
    from metrabs_amd import kernels
    fn = kernels.expand_depthwise16_planes
    x, w1, b1, wd, b2 = _inputs(2, 8, 32, 12, 12, 1, torch.float16)
    ok, okm = fn(x, w1, b1, None, wd, b2, 'relu', want_mean=True)
    want, wmean = _chain(x, w1, b1, None, wd, b2, 'relu')
    assert torch.equal(ok, want) and torch.equal(okm, wmean)
    with pytest.raises(ValueError):
        fn(x, w1[:, :4].contiguous(), b1, None, wd, b2, None)      # W1 of another Cin
    with pytest.raises(ValueError):
        fn(x, w1.bfloat16(), b1, None, wd, b2, None)
    with pytest.raises(ValueError):
        fn(x, w1, b1, None, wd[:16], b2, None)                     # Wd of another Cmid
    with pytest.raises(ValueError):
        fn(x, w1, b1[:8], None, wd, b2, None)
    with pytest.raises(ValueError):
        fn(x.to(memory_format=torch.channels_last), w1, b1, None, wd, b2, None)
    with pytest.raises(ValueError):
        fn(x, w1, b1, None, wd, b2, None, out=torch.empty_like(ok).float())
    with pytest.raises(ValueError):
        fn(x, w1, b1, None, wd, b2, None, out=ok[:, :16])
    for H, W in [(8, 8), (16, 16), (32, 16), (32, 32)]:   # MTR_E_SHAPE: K11's block-kernel planes; 1024 positions
        assert not kernels.expand_depthwise16_planes_supported(x.new_zeros(2, 8, H, W), w1)
        with pytest.raises(RuntimeError):
            fn(x.new_zeros(2, 8, H, W), w1, b1, None, wd, b2, None)
    with pytest.raises((RuntimeError, TypeError)):
        fn(x.float(), w1.float(), b1, None, wd, b2, None)
    # y overlapping x: an expand of as many channels as its input, written in place
    xs, w1s, b1s, wds, b2s = _inputs(2, 8, 8, 12, 12, 2, torch.float16)
    with pytest.raises(RuntimeError):
        fn(xs, w1s, b1s, None, wds, b2s, None, out=xs)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fn(x.cpu(), w1.cpu(), b1.cpu(), None, wd.cpu(), b2.cpu(), None)
    assert not kernels.expand_depthwise16_planes_supported(x.to(memory_format=torch.channels_last), w1)
    assert not kernels.expand_depthwise16_planes_supported(x.float(), w1)
    assert kernels.expand_depthwise16_planes_supported(x, w1)


# ---- the armed copies

def _pairs(net, field='hand_planes_to'):
    from metrabs_amd import backbones
    return [(m, getattr(m, field)[0]) for m in net.modules()
            if isinstance(m, backbones.ConvBiasAct) and getattr(m, field)]


@pytest.fixture(scope='module')
def net_s():
    return _calibrated('efficientnetv2-s', 256)


def _x(res, seed):
    return torch.rand(2, 3, res, res, device='cuda', generator=torch.Generator(device='cuda').manual_seed(seed))


def _run(net, x):
    with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        return net(x)


@pytest.mark.parametrize('dtype', DTYPES)
def test_armed_copy_takes_k26h_at_384_px_and_keeps_the_bits(dtype, net_s, hip_lib):
    from metrabs_amd import backbones
    DW = backbones.DepthwiseBiasAct
    plain = backbones.fold_batchnorm(net_s, fused_epilogue=True, dtype=dtype)
    armed = backbones.fold_batchnorm(net_s, fused_epilogue=True, dtype=dtype, fuse_expand_depthwise_planes=True)
    assert not _pairs(plain) and not _pairs(armed, 'hand_to')
    assert list(plain.state_dict()) == list(armed.state_dict())
    assert [type(m) for m in plain.modules()] == [type(m) for m in armed.modules()]
    pairs = _pairs(armed)
    assert len(pairs) == 28
    x = _x(384, 1)
    seen = {}
    hs = [e.register_forward_pre_hook(lambda mod, args: seen.__setitem__(mod, tuple(args[0].shape))) for e, _ in pairs]
    shipped = DW.k26h_slower
    key = lambda e: (seen[e][1], e.conv.out_channels, seen[e][2], seen[e][3])
    try:
        off = _run(plain, x)
        # as shipped: the classes of k26h_slower keep the chain, the others fuse; the same bits
        assert torch.equal(_run(armed, x), off)
        assert {seen[e][2:] for e, _ in pairs} == {(24, 24), (12, 12)}
        for e, d in pairs:
            fused = key(e) not in shipped
            assert (e.last_path == 'k26h') == fused == (d.last_path == 'k26h'), (key(e), e.last_path, d.last_path)
        # the list emptied: all 28 pairs run on it
        DW.k26h_slower = frozenset()
        on = _run(armed, x)
        assert torch.equal(on, off)
        assert [(e.last_path, d.last_path) for e, d in pairs] == [('k26h', 'k26h')] * 28
        with torch.inference_mode():
            assert e.path(torch.empty(seen[e], device='cuda', dtype=dtype)) == 'k26h'
        # every other layer reports what it reports in the default copy
        fused = {id(m) for p in pairs for m in p}
        assert [(type(a).__name__, getattr(a, 'last_path', None)) for a in armed.modules() if id(a) not in fused] == \
            [(type(m).__name__, getattr(m, 'last_path', None)) for m, a in zip(plain.modules(), armed.modules())
             if id(a) not in fused]
        # the class switch, and a filled k26h_slower, send every pair back to the chain
        DW.use_k26h = False
        assert torch.equal(_run(armed, x), off) and _paths(armed) == _paths(plain)
        DW.use_k26h = True
        DW.k26h_slower = frozenset(key(e) for e, _ in pairs)
        assert torch.equal(_run(armed, x), off) and _paths(armed) == _paths(plain)
        DW.k26h_slower = frozenset()
        assert torch.equal(_run(armed, x), off)
        assert sum(e.last_path == 'k26h' for e, _ in pairs) == 28
        # the same copy on a 256 px input: 16x16 and 8x8 planes are K25h's, no pair runs K26h
        x256 = _x(256, 2)
        assert torch.equal(_run(armed, x256), _run(plain, x256))
        assert _paths(armed) == _paths(plain)
        assert not any(getattr(m, 'last_path', None) == 'k26h' for m in armed.modules())
    finally:
        DW.use_k26h = True
        DW.k26h_slower = shipped
        for h in hs:
            h.remove()
    assert on.dtype == dtype and torch.isfinite(on).all()


@pytest.mark.parametrize('dtype', DTYPES)
def test_both_expand_depthwise_options_split_the_planes_between_them(dtype, net_s, hip_lib):
    from metrabs_amd import backbones
    DW = backbones.DepthwiseBiasAct
    plain = backbones.fold_batchnorm(net_s, fused_epilogue=True, dtype=dtype)
    both = backbones.fold_batchnorm(net_s, fused_epilogue=True, dtype=dtype, fuse_expand_depthwise=True,
                                    fuse_expand_depthwise_planes=True)
    pairs = _pairs(both)
    assert len(pairs) == 28 and [id(e) for e, _ in pairs] == [id(e) for e, _ in _pairs(both, 'hand_to')]
    shipped = DW.k25h_slower, DW.k26h_slower
    DW.k25h_slower = DW.k26h_slower = frozenset()
    try:
        x = _x(384, 3)
        assert torch.equal(_run(both, x), _run(plain, x))
        assert [(e.last_path, d.last_path) for e, d in pairs] == [('k26h', 'k26h')] * 28
        x = _x(256, 4)
        assert torch.equal(_run(both, x), _run(plain, x))
        assert [(e.last_path, d.last_path) for e, d in pairs] == [('k25h', 'k25h')] * 28
    finally:
        DW.k25h_slower, DW.k26h_slower = shipped


@pytest.mark.parametrize('dtype', DTYPES)
def test_k26h_with_the_other_options(dtype, net_s, hip_lib):
    """fuse_blocks, fuse_stem, block_depthwise and deep_projects touch other modules or other fields: the copy with
    all of them and fuse_expand_depthwise_planes has the bits of the copy with them alone (deep_projects itself differs
    from the default copy by rounding), K26h takes the pairs, and a pair it does not take runs K13h + K18.  Without
    deep_projects the features are the default copy's."""
    from metrabs_amd import backbones
    DW = backbones.DepthwiseBiasAct
    others = dict(fuse_blocks=True, fuse_stem=True, block_depthwise=True, deep_projects=True)
    base = backbones.fold_batchnorm(net_s, fused_epilogue=True, dtype=dtype, **others)
    both = backbones.fold_batchnorm(net_s, fused_epilogue=True, dtype=dtype, fuse_expand_depthwise_planes=True,
                                    **others)
    plain = backbones.fold_batchnorm(net_s, fused_epilogue=True, dtype=dtype)
    k18 = backbones.fold_batchnorm(net_s, fused_epilogue=True, dtype=dtype, fuse_expand_depthwise_planes=True,
                                   block_depthwise=True)
    x = _x(384, 2)
    shipped, DW.k26h_slower = DW.k26h_slower, frozenset()   # every pair the kernel takes
    try:
        want = _run(base, x)
        assert torch.equal(_run(both, x), want)
        pairs = _pairs(both)
        assert len(pairs) == 28 and [(e.last_path, d.last_path) for e, d in pairs] == [('k26h', 'k26h')] * 28
        fused = {id(m) for p in pairs for m in p}
        assert [getattr(a, 'last_path', None) for a in both.modules() if id(a) not in fused] == \
            [getattr(m, 'last_path', None) for m, a in zip(base.modules(), both.modules()) if id(a) not in fused]
        assert torch.equal(_run(k18, x), _run(plain, x))
        assert [(e.last_path, d.last_path) for e, d in _pairs(k18)] == [('k26h', 'k26h')] * 28
        DW.use_k26h = False
        assert torch.equal(_run(both, x), want) and _paths(both) == _paths(base)
        assert [(e.last_path, d.last_path) for e, d in pairs] == [('k13h', 'k18')] * 28
    finally:
        DW.use_k26h = True
        DW.k26h_slower = shipped


def test_a_refusal_after_the_hand_over_still_runs_the_expand(net_s, hip_lib):
    """Whatever changes between the expand's question and the depthwise layer's forward: a tensor never skips its
    expand."""
    from metrabs_amd import backbones
    DW = backbones.DepthwiseBiasAct
    armed = backbones.fold_batchnorm(net_s, fused_epilogue=True, dtype=torch.float16, fuse_expand_depthwise_planes=True)
    e, d = _pairs(armed)[0]
    x = torch.randn(2, e.conv.in_channels, 24, 24, device='cuda').half()
    shipped, DW.k26h_slower = DW.k26h_slower, frozenset()
    try:
        with torch.inference_mode():
            want = d(e.forward_here(x))
            assert e.hands_over(x) and e(x) is x and e.last_path == 'k26h'
            DW.use_k26h = False
            got = d(x)
            assert torch.equal(got, want) and d.last_path == 'k11' and e.last_path == 'k13h'
            DW.use_k26h = True
            assert e(x) is x
            fused = d(x)
            assert torch.equal(fused, want) and d.last_path == 'k26h'
            # a tensor that was NOT handed over is an ordinary input of the depthwise layer
            assert e(x) is x
            other = want.clone()
            assert torch.equal(d(other), d.forward(other)) and d.last_path == 'k11'
            # a 16x16 plane is not K26h's: the expand runs its own kernel
            x16 = torch.randn(2, e.conv.in_channels, 16, 16, device='cuda').half()
            assert not e.hands_over(x16) and e(x16) is not x16 and e.last_path == 'k13h'
    finally:
        DW.use_k26h = True
        DW.k26h_slower = shipped


def _model_dir(tmp_path):
    from metrabs_amd import backbones, loading
    from metrabs_amd.config import MetrabsConfig
    from metrabs_amd.joint_info import JointInfo
    from metrabs_amd.models.metrabs import Metrabs
    raw = dict(proc_side=384, stride_train=32, stride_test=32, centered_stride=True, depth=8,
               box_size_mm=2200, efficientnet_size='s', weak_perspective=False, mix_3d_inside_fov=0.5)
    bb = backbones.efficientnetv2('s')
    model = Metrabs(bb, JointInfo(cases.COCO17, cases.COCO17_EDGES), MetrabsConfig.from_any(raw),
                    in_channels=bb.out_channels)
    model.load_state_dict(cases.deterministic_state(model.state_dict(), seed=11))
    skel = {'': dict(indices=list(range(17)), names=cases.COCO17, edges=cases.COCO17_EDGES)}
    d = str(tmp_path / 'model')
    loading.save_model_dir(d, model, raw, skel, np.eye(17, dtype=np.float32))
    return d


def test_k26h_through_the_loader_and_the_api(tmp_path, hip_lib):
    from metrabs_amd import backbones, loading
    DW = backbones.DepthwiseBiasAct
    d = _model_dir(tmp_path)
    with pytest.raises(ValueError):
        loading.load_crop_model(d, fuse_expand_depthwise_planes=True)
    with pytest.raises(ValueError):
        loading.load_multiperson_model(d, fuse_expand_depthwise_planes=True)
    plain = loading.load_multiperson_model(d, dtype=torch.float16)
    plain.crop_model.deterministic_backbone = True
    plain.graph_batches = False
    est = loading.load_multiperson_model(d, dtype=torch.float16, fuse_expand_depthwise_planes=True)
    est.crop_model.deterministic_backbone = True
    est.graph_batches = True
    eager = loading.load_multiperson_model(d, dtype=torch.float16, fuse_expand_depthwise_planes=True)
    eager.crop_model.deterministic_backbone = True
    eager.graph_batches = False
    shipped, DW.k26h_slower = DW.k26h_slower, frozenset()
    try:
        for seed in (5, 9):
            images = torch.stack([cases.synth_images(1, 240, 320, seed + i)[0] for i in range(2)]).cuda()
            boxes = [torch.tensor([[60.0, 20.0, 120.0, 200.0], [150.0, 30.0, 100.0, 180.0]]),
                     torch.tensor([[40.0, 10.0, 140.0, 210.0]])]
            ref, a, b = _poses(plain, images, boxes), _poses(eager, images, boxes), _poses(est, images, boxes)
            assert torch.isfinite(a).all()
            assert torch.equal(a, ref), float((a - ref).abs().max())   # the armed copy returns the unarmed copy's bits
            assert torch.equal(a, b), float((a - b).abs().max())       # a graphed call returns the eager call's bits
    finally:
        DW.k26h_slower = shipped
    for model in (est, eager):
        pairs = _pairs(model.crop_model.backbone)
        assert len(pairs) == 28 and all(e.last_path == 'k26h' and dw.last_path == 'k26h' for e, dw in pairs)
    assert not _pairs(plain.crop_model.backbone)
    assert est.graphs.stats['captures'] >= 1 and est.graphs.stats['replays'] >= 1, est.graphs.stats

"""GPU: K27h (csrc/expand_dw16_tiles.hip) -- the 1x1 expand of an MBConv block of the 16-bit inference copy (K13h) and
the depthwise 3x3 layer behind it, stride 1 or 2, as one launch in BANDS of output rows, without a mean -- on the large
planes K25h and K26h refuse (64x64, 128x128 -> 64x64, 32x32 -> 16x16 of MobileNetV3).

Three independent checks per shape.  (a) BITS: y torch.equal to kernels.conv1x1_bias_act16 followed by
kernels.depthwise3x3_bias_act(.., stride, 1) on the same tensors -- the kernel's contract -- and, at stride 1, to
conv1x1_bias_act16 followed by kernels.depthwise3x3_blocks_bias_act (K18), which has the generic kernel's bits too.
(b) fp64, independently of the chain: the two layers in float64 on the 16-bit operands, the intermediate NOT rounded.
(c) small integers, exact.

The fp64 bound at stride 1 is the one of tests/test_gpu_expand_dw16.py (its code is imported from there, unchanged).
u = 2^-24, u_out = one rounding of the 16-bit format (2^-11 f16, 2^-8 bf16), ulp(v) = one unit in the last place of the
format at |v|, L(act) the activation's Lipschitz constant (1 none and relu, 1.1 silu, 1.5 hardswish).  With z1 = W1 x +
b1, s1 = |W1| |x| + |b1|, m = act1(z1), per position of the INPUT plane:

    d_mid = ulp(m) + L(act1) * Cin * u * s1 + 1e-6 |m| + u

The stride-2 form, derived the same way before the kernel first ran: an output o of the stride-2 layer is the same
eleven operations (nine fma and the bias, whatever their order) through the same activation and one output rounding,
over the window of the intermediate centred on input position 2 o, zero outside the plane.  Nothing in section 30's
derivation uses where the window sits, so the three window sums are taken at stride 2 and everything else stands: with
v = b2 + sum_{window of 2 o} Wd m (fp64, m unrounded), c = sum_{window} |Wd| d_mid, S = sum_{window} |Wd| (|m| + d_mid)
+ |b2| and ref = act2(v):

    E     = 1.5 * 11 u S + (8 + 2 (|v| + c)) u (|ref| + L(act2) c)
    bound = (L(act2) c + E) (1 + u_out) + u_out |ref| + tiny          (tiny = 2^-25 f16, 2^-126 bf16)

Every element is checked; the largest error as a share of the bound is printed (DESIGN.md section 32 records it).
Then: every activation pair on one shape per stride, determinism, out=, graph replay, guard bands, the wrapper's
refusals; the armed copies of MobileNetV3 and EfficientNetV2-S at 256 px (paths, switches, the other options, K25h's and
K26h's among them); the loader and the API on a MobileNetV3 model."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cases
from test_gpu_expand_dw16 import (_LIPSCHITZ, ACTS, DTYPES, TINY, U, U_OUT, _act64, _calibrated, _check_fp64, _inputs,
                                  _paths, _poses, _ulp)

pytestmark = pytest.mark.gpu

# (stride, Cin, Cmid, H, W, the batch sizes): the smallest shapes that hit more than one band, a partial last band, the
# k tail and a partial channel chunk; the three classes of MobileNetV3 at 256 px with B = 1
SHAPES = [
    (1, 8, 8, 12, 12, (1, 3)),       # bands of 8 + 4 rows; a quarter of a channel chunk
    (1, 24, 40, 20, 8, (1, 3)),      # 8 + 8 + 4 rows of 8: segments of eight outputs; half a k step; two chunks
    (1, 16, 72, 36, 36, (1, 3)),     # W % 8 == 4: the staged span starts four positions early; three chunks
    (1, 40, 200, 28, 24, (1, 3)),    # two k-tiles, the second a quarter full; seven chunks, the last of 8 channels
    (1, 24, 72, 64, 64, (1,)),       # the real class: ten bands of 6 rows and one of 4
    (2, 8, 8, 8, 8, (1, 3)),         # one band; segments of four outputs
    (2, 24, 40, 12, 16, (1, 3)),     # bands of 4 + 2 output rows
    (2, 16, 24, 6, 24, (1, 3)),      # H / 2 odd, one band of 3 rows; W / 2 % 8 == 4
    (2, 40, 240, 32, 32, (1,)),      # the real class: four bands of 4 rows, segments of eight
    (2, 16, 64, 128, 128, (1,)),     # the real class: 1024 staged positions, 21 bands of 3 rows and one of 1
]
CASES = [(s, K, M, H, W, B) for s, K, M, H, W, Bs in SHAPES for B in Bs]


def _chain(x, w1, b1, act1, wd, b2, act2, stride):
    from metrabs_amd import kernels
    mid = kernels.conv1x1_bias_act16(x, w1, b1, act1)
    return kernels.depthwise3x3_bias_act(mid, wd, b2, act2, stride, 1)


def _k18_chain(x, w1, b1, act1, wd, b2, act2):
    from metrabs_amd import kernels
    mid = kernels.conv1x1_bias_act16(x, w1, b1, act1)
    return kernels.depthwise3x3_blocks_bias_act(mid, wd, b2, act2)


def _reference_s2(x, w1, b1, act1, wd, b2, act2):
    """(fp64 result, the module docstring's stride-2 bound): test_gpu_expand_dw16._reference with the three window sums
    taken at stride 2."""
    dt = x.dtype
    Cin, Cmid = x.shape[1], w1.shape[0]
    w1d = w1.double()[:, :, None, None]
    z1 = F.conv2d(x.double(), w1d) + b1.double()[None, :, None, None]
    s1 = F.conv2d(x.double().abs(), w1d.abs()) + b1.double().abs()[None, :, None, None]
    m = _act64(z1, act1)
    d_mid = _ulp(m, dt) + _LIPSCHITZ[act1] * Cin * U * s1 + 1e-6 * m.abs() + U
    wdd, b2d = wd.double().reshape(Cmid, 1, 3, 3), b2.double()[None, :, None, None]
    v = F.conv2d(m, wdd, None, 2, 1, groups=Cmid) + b2d
    c = F.conv2d(d_mid, wdd.abs(), None, 2, 1, groups=Cmid)
    S = F.conv2d(m.abs() + d_mid, wdd.abs(), None, 2, 1, groups=Cmid) + b2d.abs()
    ref = _act64(v, act2)
    L2 = _LIPSCHITZ[act2]
    E = 1.5 * 11 * U * S + (8 + 2 * (v.abs() + c)) * U * (ref.abs() + L2 * c)
    return ref, (L2 * c + E) * (1 + U_OUT[dt]) + U_OUT[dt] * ref.abs() + TINY[dt]


def _check(x, w1, b1, act1, wd, b2, act2, stride, got, label):
    if stride == 1:
        return _check_fp64(x, w1, b1, act1, wd, b2, act2, got, None, 'k27h ' + label)
    ref, bound = _reference_s2(x, w1, b1, act1, wd, b2, act2)
    assert got.shape == ref.shape and got.dtype == x.dtype
    err = (got.double() - ref).abs()
    print(f'k27h fp64 stride 2 {label} {x.dtype}: max err / bound = {float((err / bound).max()):.3f}')
    assert float((err - bound).max()) <= 0


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', CASES, ids=lambda c: 's{}-{}-{}-{}x{}-B{}'.format(*c))
def test_k27h_has_the_chains_bits_and_meets_the_fp64_bound(case, dtype, hip_lib):
    from metrabs_amd import kernels
    stride, Cin, Cmid, H, W, B = case
    x, w1, b1, wd, b2 = _inputs(B, Cin, Cmid, H, W, 100 + Cin + H, dtype)
    assert kernels.expand_depthwise16_tiles_supported(x, w1, stride), case
    assert kernels.conv1x1_16_supported(x, w1)
    assert stride == 2 or not kernels.k11_takes_block_kernel(H, W)
    got = kernels.expand_depthwise16_tiles(x, w1, b1, 'silu', wd, b2, 'silu', stride)
    assert isinstance(got, torch.Tensor) and got.shape == (B, Cmid, H // stride, W // stride)
    chains = [('k11', _chain(x, w1, b1, 'silu', wd, b2, 'silu', stride))]
    if stride == 1:
        chains.append(('k18', _k18_chain(x, w1, b1, 'silu', wd, b2, 'silu')))
    for name, want in chains:
        diff = (got.float() - want.float()).abs()
        assert torch.equal(got, want), (name, case, int((got != want).sum()), float(diff.max()))
    _check(x, w1, b1, 'silu', wd, b2, 'silu', stride, got, f'{case}')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('stride', [1, 2])
def test_k27h_every_activation_pair(stride, dtype, hip_lib):
    from metrabs_amd import kernels
    Cin, Cmid, H, W = (24, 40, 20, 8) if stride == 1 else (24, 40, 12, 16)
    x, w1, b1, wd, b2 = _inputs(3, Cin, Cmid, H, W, 11, dtype)
    for act1 in ACTS:
        for act2 in ACTS:
            want = _chain(x, w1, b1, act1, wd, b2, act2, stride)
            got = kernels.expand_depthwise16_tiles(x, w1, b1, act1, wd, b2, act2, stride)
            assert torch.equal(got, want), (act1, act2, int((got != want).sum()))
            _check(x, w1, b1, act1, wd, b2, act2, stride, got, f'{Cin}-{Cmid} {H}x{W} {act1}/{act2}')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('act', [None, 'relu'])
@pytest.mark.parametrize('stride,shape', [(1, (24, 72, 20, 12)), (2, (24, 72, 12, 16))])
def test_k27h_is_exact_on_small_integers(stride, shape, act, dtype, hip_lib):
    """Small-integer data, an expand that looks at two input channels per output channel and an asymmetric depthwise
    weight (every tap distinct): every product, every partial sum, the intermediate and the output are integers of at
    most 2^8 in magnitude (exact in bf16, hence in f16), checked here on the reference -- so the result must EQUAL
    the integer evaluation: a swapped tap, a transposed fragment, a wrong band, chunk or halo row cannot hide in
    rounding.  Both shapes are three chunks of channels, the last one partial, and more than one band."""
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
    ref = _act64(F.conv2d(mid, wd.double(), b2.double(), stride, 1, groups=Cmid), act)
    assert float(mid.abs().max()) <= 5 and float(ref.abs().max()) <= 16 * 5 + 3 <= 2 ** 8
    assert float(ref.abs().max()) > 15   # (more than one tap can give, 3 * 5: not a trivially small case)
    got = kernels.expand_depthwise16_tiles(x.to(dtype), w1.to(dtype), b1, act, wd, b2, act, stride)
    assert torch.equal(got.double(), ref)


@pytest.mark.parametrize('dtype', DTYPES)
def test_k27h_is_deterministic_graph_safe_and_stays_inside_y(dtype, hip_lib):
    from metrabs_amd import kernels
    fn = kernels.expand_depthwise16_tiles
    # B = 9: the grid is padded to 16 images, and workgroups past the batch leave at once
    for (B, Cin, Cmid, H, W, stride) in [(9, 16, 72, 36, 36, 1), (2, 24, 40, 12, 16, 2), (9, 8, 8, 8, 8, 2)]:
        x, w1, b1, wd, b2 = _inputs(B, Cin, Cmid, H, W, 5, dtype)
        a = fn(x, w1, b1, 'silu', wd, b2, 'silu', stride)
        assert torch.equal(a, fn(x, w1, b1, 'silu', wd, b2, 'silu', stride))
        assert torch.equal(a, _chain(x, w1, b1, 'silu', wd, b2, 'silu', stride))
        # out= inside guard bands (64 elements either side: y's base stays 16-byte aligned)
        flat = torch.full((a.numel() + 128,), 7.0, device='cuda', dtype=dtype)
        out = flat[64:64 + a.numel()].view_as(a)
        assert fn(x, w1, b1, 'silu', wd, b2, 'silu', stride, out=out) is out
        assert torch.equal(out, a)
        assert bool((flat[:64] == 7.0).all()) and bool((flat[-64:] == 7.0).all())
        with torch.inference_mode():
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                fn(x, w1, b1, 'silu', wd, b2, 'silu', stride, out=out)
                st.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                    fn(x, w1, b1, 'silu', wd, b2, 'silu', stride, out=out)
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
        assert kernels.expand_depthwise16_tiles_supported(x8, w1, stride)
        assert torch.equal(fn(x8, w1, b1, 'silu', wd, b2, 'silu', stride), a)
        x4 = xflat[4:4 + x.numel()].view_as(x)
        assert not kernels.expand_depthwise16_tiles_supported(x4, w1, stride)
        with pytest.raises(RuntimeError):
            fn(x4, w1, b1, 'silu', wd, b2, 'silu', stride)


def test_k27h_wrapper_argument_checks(hip_lib):
    from metrabs_amd import kernels
    fn, ask = kernels.expand_depthwise16_tiles, kernels.expand_depthwise16_tiles_supported
    x, w1, b1, wd, b2 = _inputs(2, 8, 32, 12, 12, 1, torch.float16)
    ok = fn(x, w1, b1, None, wd, b2, 'relu')
    assert torch.equal(ok, _chain(x, w1, b1, None, wd, b2, 'relu', 1))
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
    with pytest.raises(ValueError):
        fn(x, w1, b1, None, wd, b2, None, stride=2, out=ok)        # the stride-2 output is [.., 6, 6]
    with pytest.raises(ValueError):
        fn(x, w1, b1, None, wd, b2, None, stride=3)
    for H, W in [(8, 8), (16, 16), (32, 16), (16, 32), (32, 32)]:   # MTR_E_SHAPE at stride 1: K11's block-kernel planes
        assert not ask(x.new_zeros(2, 8, H, W), w1) and ask(x.new_zeros(2, 8, H, W), w1, 2)
        with pytest.raises(RuntimeError):
            fn(x.new_zeros(2, 8, H, W), w1, b1, None, wd, b2, None)
    for H, W in [(7, 8), (9, 16), (8, 12), (8, 20)]:   # stride 2: odd H; W % 8 != 0
        assert not ask(x.new_zeros(2, 8, H, W), w1, 2)
        with pytest.raises(RuntimeError):
            fn(x.new_zeros(2, 8, H, W), w1, b1, None, wd, b2, None, stride=2)
    with pytest.raises((RuntimeError, TypeError)):
        fn(x.float(), w1.float(), b1, None, wd, b2, None)
    # a misaligned x
    xflat = torch.zeros(x.numel() + 8, device='cuda', dtype=torch.float16)
    with pytest.raises(RuntimeError):
        fn(xflat[4:4 + x.numel()].view_as(x), w1, b1, None, wd, b2, None)
    # y overlapping x: an expand of as many channels as its input, written in place
    xs, w1s, b1s, wds, b2s = _inputs(2, 8, 8, 12, 12, 2, torch.float16)
    with pytest.raises(RuntimeError):
        fn(xs, w1s, b1s, None, wds, b2s, None, out=xs)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fn(x.cpu(), w1.cpu(), b1.cpu(), None, wd.cpu(), b2.cpu(), None)
    assert not ask(x.to(memory_format=torch.channels_last), w1)
    assert not ask(x.float(), w1) and not ask(x.float(), w1, 2)
    assert ask(x, w1) and not ask(x, w1, 2) and ask(x.new_zeros(2, 8, 12, 16), w1, 2)   # (12 % 8 != 0)


# ---- the armed copies

FIELD = 'hand_tiles_to'
# the classes of MobileNetV3 at 256 px that K27h is for: (Cin, Cmid, H, W, stride) of the expand's input
K27H_CLASSES = {(24, 72, 64, 64, 1), (16, 64, 128, 128, 2), (40, 240, 32, 32, 2)}


def _pairs(net, field=FIELD):
    from metrabs_amd import backbones
    return [(m, getattr(m, field)[0]) for m in net.modules()
            if isinstance(m, backbones.ConvBiasAct) and getattr(m, field)]


@pytest.fixture(scope='module')
def nets():
    return {name: _calibrated(name, 256) for name in ('efficientnetv2-s', 'mobilenetv3')}


def _x(res, seed):
    return torch.rand(2, 3, res, res, device='cuda', generator=torch.Generator(device='cuda').manual_seed(seed))


def _run(net, x):
    with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        return net(x)


def _watch(pairs):
    seen = {}
    hooks = [e.register_forward_pre_hook(lambda mod, args: seen.__setitem__(mod, tuple(args[0].shape)))
             for e, _ in pairs]
    return seen, hooks


@pytest.mark.parametrize('dtype', DTYPES)
def test_armed_mobilenetv3_takes_k27h_on_its_three_classes_and_keeps_the_bits(dtype, nets, hip_lib):
    from metrabs_amd import backbones
    DW = backbones.DepthwiseBiasAct
    plain = backbones.fold_batchnorm(nets['mobilenetv3'], fused_epilogue=True, dtype=dtype)
    armed = backbones.fold_batchnorm(nets['mobilenetv3'], fused_epilogue=True, dtype=dtype,
                                     fuse_expand_depthwise_tiles=True)
    assert not _pairs(plain) and not _pairs(armed, 'hand_to') and not _pairs(armed, 'hand_planes_to')
    assert list(plain.state_dict()) == list(armed.state_dict())
    assert [type(m) for m in plain.modules()] == [type(m) for m in armed.modules()]
    pairs = _pairs(armed)
    assert len(pairs) == 8 and sorted(d.stride for _, d in pairs) == [1] * 6 + [2] * 2
    x = _x(256, 1)
    seen, hs = _watch(pairs)
    shipped = DW.k27h_slower
    key = lambda e, d: (seen[e][1], e.conv.out_channels, seen[e][2], seen[e][3], d.stride)
    try:
        off = _run(plain, x)
        # as shipped: the classes of k27h_slower keep the chain, the others fuse; the same bits
        assert torch.equal(_run(armed, x), off)
        assert {key(e, d) for e, d in pairs if seen[e][2] > 16} == K27H_CLASSES
        for e, d in pairs:
            fused = key(e, d) in K27H_CLASSES and key(e, d) not in shipped
            assert (e.last_path == 'k27h') == fused == (d.last_path == 'k27h'), (key(e, d), e.last_path, d.last_path)
        # the list emptied: the three classes run on it, the five 16x16 pairs keep what they ran
        DW.k27h_slower = frozenset()
        on = _run(armed, x)
        assert torch.equal(on, off)
        for e, d in pairs:
            with torch.inference_mode():
                asked = e.path(torch.empty(seen[e], device='cuda', dtype=dtype))
            if key(e, d) in K27H_CLASSES:
                assert (e.last_path, d.last_path, asked) == ('k27h', 'k27h', 'k27h'), (key(e, d), e.last_path)
            else:   # (compared with the default copy's paths below)
                assert 'k27h' not in (e.last_path, d.last_path, asked) and d.last_path == 'k11', key(e, d)
        assert sum(key(e, d) not in K27H_CLASSES and seen[e][2:] == (16, 16) for e, d in pairs) == 5
        # every other layer reports what it reports in the default copy
        fused = {id(m) for p in pairs if key(*p) in K27H_CLASSES for m in p}
        assert [(type(a).__name__, getattr(a, 'last_path', None)) for a in armed.modules() if id(a) not in fused] == \
            [(type(m).__name__, getattr(m, 'last_path', None)) for m, a in zip(plain.modules(), armed.modules())
             if id(a) not in fused]
        # the class switch, and a filled k27h_slower, send every pair back to the chain
        DW.use_k27h = False
        assert torch.equal(_run(armed, x), off) and _paths(armed) == _paths(plain)
        DW.use_k27h = True
        DW.k27h_slower = frozenset(key(e, d) for e, d in pairs)
        assert torch.equal(_run(armed, x), off) and _paths(armed) == _paths(plain)
        DW.k27h_slower = frozenset()
        assert torch.equal(_run(armed, x), off)
        assert sum(e.last_path == 'k27h' for e, _ in pairs) == 3
    finally:
        DW.use_k27h = True
        DW.k27h_slower = shipped
        for h in hs:
            h.remove()
    assert on.dtype == dtype and torch.isfinite(on).all()


@pytest.mark.parametrize('dtype', DTYPES)
def test_armed_efficientnetv2_s_runs_no_pair_on_k27h(dtype, nets, hip_lib):
    """Every MBConv block of EfficientNetV2 has a squeeze-excite block: its depthwise layer emits the mean, which K27h
    does not have.  28 pairs are armed (fuse_expand_depthwise's), none is taken."""
    from metrabs_amd import backbones
    DW = backbones.DepthwiseBiasAct
    plain = backbones.fold_batchnorm(nets['efficientnetv2-s'], fused_epilogue=True, dtype=dtype)
    armed = backbones.fold_batchnorm(nets['efficientnetv2-s'], fused_epilogue=True, dtype=dtype,
                                     fuse_expand_depthwise_tiles=True)
    pairs = _pairs(armed)
    assert len(pairs) == 28 and all(d.stride == 1 and d.emit_mean for _, d in pairs)
    shipped, DW.k27h_slower = DW.k27h_slower, frozenset()
    try:
        x = _x(256, 2)
        assert torch.equal(_run(armed, x), _run(plain, x))
        assert _paths(armed) == _paths(plain)
        assert not any(getattr(m, 'last_path', None) == 'k27h' for m in armed.modules())
    finally:
        DW.k27h_slower = shipped


@pytest.mark.parametrize('dtype', DTYPES)
def test_k27h_beside_the_other_expand_depthwise_options_and_block_depthwise(dtype, nets, hip_lib):
    """fuse_expand_depthwise (K25h), fuse_expand_depthwise_planes (K26h) and block_depthwise (K18) beside the new option:
    separate fields, disjoint planes.  Every pair has the path it has with its own option alone -- the three large
    classes K27h, the 16x16 pairs whatever the K25h-armed copy runs there -- and the features are the default copy's.
    With K27h switched off the stride-1 64x64 pair runs K13h + K18 and the stride-2 pairs K13h + K11."""
    from metrabs_amd import backbones
    DW = backbones.DepthwiseBiasAct
    net = nets['mobilenetv3']
    plain = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype)
    k25h = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, fuse_expand_depthwise=True)
    all4 = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, fuse_expand_depthwise=True,
                                    fuse_expand_depthwise_planes=True, fuse_expand_depthwise_tiles=True,
                                    block_depthwise=True)
    pairs = _pairs(all4)
    assert len(pairs) == 8 and len(_pairs(all4, 'hand_to')) == 6 == len(_pairs(all4, 'hand_planes_to'))
    x = _x(256, 3)
    seen, hs = _watch(pairs)
    shipped, DW.k27h_slower = DW.k27h_slower, frozenset()
    try:
        off = _run(plain, x)
        assert torch.equal(_run(k25h, x), off)
        alone = {id(d): (e.last_path, d.last_path) for e, d in _pairs(k25h, 'hand_to')}
        by_place = dict(zip((id(d) for _, d in _pairs(all4, 'hand_to')), (id(d) for _, d in _pairs(k25h, 'hand_to'))))
        assert torch.equal(_run(all4, x), off)
        for e, d in pairs:
            key = (seen[e][1], e.conv.out_channels, seen[e][2], seen[e][3], d.stride)
            if key in K27H_CLASSES:
                assert (e.last_path, d.last_path) == ('k27h', 'k27h'), key
            else:   # a 16x16 pair: K25h's where the K25h-armed copy fuses it, the chain (K11's block kernel) elsewhere
                assert (e.last_path, d.last_path) == alone[by_place[id(d)]], key
        assert any(p == ('k25h', 'k25h') for p in alone.values())
        assert not any(getattr(m, 'last_path', None) == 'k26h' for m in all4.modules())
        DW.use_k27h = False
        assert torch.equal(_run(all4, x), off)
        for e, d in pairs:
            key = (seen[e][1], e.conv.out_channels, seen[e][2], seen[e][3], d.stride)
            if key in K27H_CLASSES:
                want = 'k11' if d.stride == 2 else ('k18' if d._k18_takes(torch.empty(
                    seen[e][0], key[1], key[2], key[3], device='cuda', dtype=dtype)) else 'k11')
                assert (e.last_path, d.last_path) == ('k13h', want), (key, e.last_path, d.last_path)
    finally:
        DW.use_k27h = True
        DW.k27h_slower = shipped
        for h in hs:
            h.remove()


def test_a_refusal_after_the_hand_over_still_runs_the_expand(nets, hip_lib):
    """Whatever changes between the expand's question and the depthwise layer's forward: a tensor never skips its
    expand."""
    from metrabs_amd import backbones
    DW = backbones.DepthwiseBiasAct
    armed = backbones.fold_batchnorm(nets['mobilenetv3'], fused_epilogue=True, dtype=torch.float16,
                                     fuse_expand_depthwise_tiles=True)
    shipped, DW.k27h_slower = DW.k27h_slower, frozenset()
    try:
        for e, d in _pairs(armed):
            if (e.conv.in_channels, d.stride) not in ((24, 1), (40, 2)):
                continue
            side = 64 if d.stride == 1 else 32
            x = torch.randn(2, e.conv.in_channels, side, side, device='cuda').half()
            with torch.inference_mode():
                want = d(e.forward_here(x))
                assert e.hands_over(x) and e(x) is x and e.last_path == 'k27h'
                DW.use_k27h = False
                got = d(x)
                assert torch.equal(got, want) and d.last_path == 'k11' and e.last_path == 'k13h'
                DW.use_k27h = True
                assert e(x) is x
                fused = d(x)
                assert torch.equal(fused, want) and d.last_path == 'k27h'
                # a tensor that was NOT handed over is an ordinary input of the depthwise layer
                assert e(x) is x
                other = e.forward_here(x).clone()
                assert torch.equal(d(other), want) and d.last_path == 'k11'
                if d.stride == 1:   # a 16x16 plane is K11's block kernel's: the expand runs its own kernel
                    x16 = torch.randn(2, e.conv.in_channels, 16, 16, device='cuda').half()
                    assert not e.hands_over(x16) and e(x16) is not x16 and e.last_path == 'k13h'
    finally:
        DW.use_k27h = True
        DW.k27h_slower = shipped


def _model_dir(tmp_path, bb):
    from metrabs_amd import loading
    from metrabs_amd.config import MetrabsConfig
    from metrabs_amd.joint_info import JointInfo
    from metrabs_amd.models.metrabs import Metrabs
    raw = dict(proc_side=256, stride_train=32, stride_test=32, centered_stride=True, depth=8,
               box_size_mm=2200, backbone='mobilenetv3', weak_perspective=False, mix_3d_inside_fov=0.5)
    torch.manual_seed(11)
    model = Metrabs(bb, JointInfo(cases.COCO17, cases.COCO17_EDGES), MetrabsConfig.from_any(raw),
                    in_channels=bb.out_channels)
    skel = {'': dict(indices=list(range(17)), names=cases.COCO17, edges=cases.COCO17_EDGES)}
    d = str(tmp_path / 'model')
    loading.save_model_dir(d, model, raw, skel, np.eye(17, dtype=np.float32))
    return d


def test_k27h_through_the_loader_and_the_api(tmp_path, hip_lib):
    from metrabs_amd import backbones, loading
    DW = backbones.DepthwiseBiasAct
    d = _model_dir(tmp_path, _calibrated('mobilenetv3', 256).cpu())
    with pytest.raises(ValueError):
        loading.load_crop_model(d, fuse_expand_depthwise_tiles=True)
    with pytest.raises(ValueError):
        loading.load_multiperson_model(d, fuse_expand_depthwise_tiles=True)
    plain = loading.load_multiperson_model(d, dtype=torch.float16)
    plain.crop_model.deterministic_backbone = True
    plain.graph_batches = False
    est = loading.load_multiperson_model(d, dtype=torch.float16, fuse_expand_depthwise_tiles=True)
    est.crop_model.deterministic_backbone = True
    est.graph_batches = True
    eager = loading.load_multiperson_model(d, dtype=torch.float16, fuse_expand_depthwise_tiles=True)
    eager.crop_model.deterministic_backbone = True
    eager.graph_batches = False
    shipped, DW.k27h_slower = DW.k27h_slower, frozenset()
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
        DW.k27h_slower = shipped
    for model in (est, eager):
        pairs = _pairs(model.crop_model.backbone)
        assert len(pairs) == 8
        assert sum(e.last_path == 'k27h' and dw.last_path == 'k27h' for e, dw in pairs) == 3
    assert not _pairs(plain.crop_model.backbone)
    assert est.graphs.stats['captures'] >= 1 and est.graphs.stats['replays'] >= 1, est.graphs.stats

"""GPU: K25h (csrc/expand_dw16.hip), the 1x1 expand of an MBConv block of the 16-bit inference copy (K13h) and the
stride-1 depthwise 3x3 layer behind it (K11's block kernel) as one launch with the expanded activation in LDS.

Three independent checks per shape.  (1) BITS: y and the mean torch.equal to kernels.conv1x1_bias_act16 followed by
kernels.depthwise3x3_bias_act(.., 1, 1, want_mean=True) on the same tensors -- the kernel's contract.  (2) fp64,
independently of the chain: the two layers in float64 on the 16-bit operands, the intermediate NOT rounded.
(3) small integers, exact.

The fp64 bound.  u = 2^-24, u_out = one rounding of the 16-bit format (2^-11 f16, 2^-8 bf16), ulp(v) = one unit in the
last place of the format at |v|, L(act) the activation's Lipschitz constant (1 none and relu, 1.1 silu, 1.5
hardswish; test_gpu_fused_mbconv16.py's table).  With z1 = W1 x + b1, s1 = |W1| |x| + |b1|, m = act1(z1):

    d_mid = ulp(m) + L(act1) * Cin * u * s1 + 1e-6 |m| + u
            (K13h's bound in the form of DESIGN.md section 12 and test_gpu_fused_mbconv16.py: f32 accumulation over
            K = Cin through the activation, then ONE 16-bit rounding of the intermediate)

The depthwise layer then sees m + e with |e| <= d_mid.  With v = b2 + sum Wd m (fp64, m unrounded),
c = sum |Wd| d_mid (the intermediate's error carried through the nine taps), S = sum |Wd| (|m| + d_mid) + |b2| (what
every partial sum of the kernel's fma chain is bounded by) and ref = act2(v):

    E     = 1.5 * 11 u S + (8 + 2 (|v| + c)) u (|ref| + L(act2) c)
            (K11's own bound of test_gpu_depthwise3x3.py -- nine fma and the bias through an activation evaluated in
            f32 -- taken at the perturbed pre-activation, which lies within c of v)
    bound = (L(act2) c + E) (1 + u_out) + u_out |ref| + tiny
            (the carried error through act2, K11's error, one output rounding; tiny = 2^-25 f16, 2^-126 bf16)

The mean is the f32 sum of the H W STORED outputs times the rounded 1 / (H W): K11's mean bound,
|mean_hat - mean(y)| <= (H W + 1) u mean |y| + 2^-126.

Every element is checked; the largest error as a share of the bound is printed (DESIGN.md section 30 records it).
Then: every activation pair, determinism, out=, graph replay, guard bands, the argument rules; the armed copies of
EfficientNetV2-S and MobileNetV3 (paths, switches, the other options); the loader and the API."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cases

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
ACTS = [None, 'relu', 'silu', 'hardswish']
_MANT = {torch.float16: 10, torch.bfloat16: 7}
_LIPSCHITZ = {None: 1.0, 'relu': 1.0, 'silu': 1.1, 'hardswish': 1.5}
U = 2.0 ** -24
U_OUT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TINY = {torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -126}

# (Cin, Cmid, H, W): the smallest shapes at which each mechanism can go wrong
SHAPES = [
    (64, 256, 16, 16),    # several chunks; 16 lanes per plane
    (40, 72, 8, 8),       # a k tail that is half an MFMA step; a partial channel chunk; 4 lanes per plane
    (8, 8, 4, 4),         # one lane per plane and no shuffle; fewer channels than a tile
    (24, 96, 8, 16),      # rectangular planes: a transposed index shows
    (24, 96, 16, 4),
    (160, 200, 16, 16),   # ten k steps; Cmid no multiple of 32 or 64
    (256, 136, 8, 8),     # the deepest k of the networks; a chunk tail of 8 channels
]


def _act64(v, act):
    if act == 'relu':
        return v.clamp_min(0)
    if act == 'silu':
        return v * torch.sigmoid(v)
    if act == 'hardswish':
        return v * (v + 3).clamp(0, 6) / 6
    return v


def _inputs(B, Cin, Cmid, H, W, seed, dtype, border=8.0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(B, Cin, H, W, device='cuda', generator=g)
    edge = torch.ones(H, W, device='cuda')   # large border pixels: a wrong halo or padding element shows
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = border
    x = (x * edge).to(dtype)
    w1 = (torch.randn(Cmid, Cin, device='cuda', generator=g) / Cin ** 0.5).to(dtype)
    b1 = 0.5 * torch.randn(Cmid, device='cuda', generator=g)
    wd = torch.randn(Cmid, 1, 3, 3, device='cuda', generator=g) * 0.4
    b2 = torch.randn(Cmid, device='cuda', generator=g)
    return x, w1, b1, wd, b2


def _chain(x, w1, b1, act1, wd, b2, act2):
    from metrabs_amd import kernels
    mid = kernels.conv1x1_bias_act16(x, w1, b1, act1)
    return kernels.depthwise3x3_bias_act(mid, wd, b2, act2, 1, 1, want_mean=True)


def _ulp(v, dt):
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(torch.finfo(dt).tiny))) - _MANT[dt])


def _reference(x, w1, b1, act1, wd, b2, act2):
    """(fp64 result, the module docstring's bound)."""
    dt = x.dtype
    Cin, Cmid = x.shape[1], w1.shape[0]
    w1d = w1.double()[:, :, None, None]
    z1 = F.conv2d(x.double(), w1d) + b1.double()[None, :, None, None]
    s1 = F.conv2d(x.double().abs(), w1d.abs()) + b1.double().abs()[None, :, None, None]
    m = _act64(z1, act1)
    d_mid = _ulp(m, dt) + _LIPSCHITZ[act1] * Cin * U * s1 + 1e-6 * m.abs() + U
    wdd, b2d = wd.double().reshape(Cmid, 1, 3, 3), b2.double()[None, :, None, None]
    v = F.conv2d(m, wdd, None, 1, 1, groups=Cmid) + b2d
    c = F.conv2d(d_mid, wdd.abs(), None, 1, 1, groups=Cmid)
    S = F.conv2d(m.abs() + d_mid, wdd.abs(), None, 1, 1, groups=Cmid) + b2d.abs()
    ref = _act64(v, act2)
    L2 = _LIPSCHITZ[act2]
    E = 1.5 * 11 * U * S + (8 + 2 * (v.abs() + c)) * U * (ref.abs() + L2 * c)
    return ref, (L2 * c + E) * (1 + U_OUT[dt]) + U_OUT[dt] * ref.abs() + TINY[dt]


def _check_fp64(x, w1, b1, act1, wd, b2, act2, got, mean, label):
    dt = x.dtype
    ref, bound = _reference(x, w1, b1, act1, wd, b2, act2)
    assert got.shape == ref.shape and got.dtype == dt
    err = (got.double() - ref).abs()
    share = float((err / bound).max())
    mshare = 0.0
    if mean is not None:
        hw = got.shape[2] * got.shape[3]
        yd = got.double()
        mbound = (hw + 1) * U * yd.abs().mean((2, 3)) + 2.0 ** -126
        assert mean.shape == got.shape[:2] and mean.dtype == torch.float32
        mshare = float(((mean.double() - yd.mean((2, 3))).abs() / mbound).max())
    print(f'k25h fp64 {label} {dt}: max err / bound = {share:.3f}, of the mean\'s = {mshare:.3f}')
    assert float((err - bound).max()) <= 0 and mshare <= 1.0, (share, mshare)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_k25h_has_the_chains_bits_and_meets_the_fp64_bound(shape, B, dtype, hip_lib):
    from metrabs_amd import kernels
    Cin, Cmid, H, W = shape
    x, w1, b1, wd, b2 = _inputs(B, Cin, Cmid, H, W, 100 + Cin + H, dtype)
    assert kernels.expand_depthwise16_supported(x, w1), shape
    assert kernels.conv1x1_16_supported(x, w1) and kernels.k11_takes_block_kernel(H, W)
    got, mean = kernels.expand_depthwise16(x, w1, b1, 'silu', wd, b2, 'silu', want_mean=True)
    want, wmean = _chain(x, w1, b1, 'silu', wd, b2, 'silu')
    diff = (got.float() - want.float()).abs()
    assert torch.equal(got, want), (shape, int((got != want).sum()), float(diff.max()))
    assert torch.equal(mean, wmean), (shape, int((mean != wmean).sum()))
    _check_fp64(x, w1, b1, 'silu', wd, b2, 'silu', got, mean, f'{shape} B={B}')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('act2', ACTS)
@pytest.mark.parametrize('act1', ACTS)
def test_k25h_every_activation_pair_with_and_without_the_mean(act1, act2, dtype, hip_lib):
    from metrabs_amd import kernels
    x, w1, b1, wd, b2 = _inputs(3, 40, 72, 8, 8, 11, dtype)
    want, wmean = _chain(x, w1, b1, act1, wd, b2, act2)
    got, mean = kernels.expand_depthwise16(x, w1, b1, act1, wd, b2, act2, want_mean=True)
    assert torch.equal(got, want) and torch.equal(mean, wmean)
    _check_fp64(x, w1, b1, act1, wd, b2, act2, got, mean, f'40-72 8x8 {act1}/{act2}')
    alone = kernels.expand_depthwise16(x, w1, b1, act1, wd, b2, act2)
    assert isinstance(alone, torch.Tensor) and torch.equal(alone, want)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('act', [None, 'relu'])
def test_k25h_is_exact_on_small_integers(act, dtype, hip_lib):
    """Small-integer data, an expand that looks at two input channels per output channel and an asymmetric depthwise
    weight (every tap distinct): every product, every partial sum, the intermediate and the output are integers of at
    most 2^8 in magnitude (exact in bf16, hence in f16), checked here on the reference -- so the result must EQUAL
    the integer evaluation: a swapped tap, a transposed fragment, a wrong chunk or halo cannot hide in rounding.
    Cmid = 200 at 16x16 is four chunks, the last one partial."""
    from metrabs_amd import kernels
    Cin, Cmid, H, W = 24, 200, 16, 16
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
    got, mean = kernels.expand_depthwise16(x.to(dtype), w1.to(dtype), b1, act, wd, b2, act, want_mean=True)
    assert torch.equal(got.double(), ref)
    # 256 integers of at most 2^7: every partial sum is exact in f32; 1 / 256 is a power of two
    assert torch.equal(mean.double(), ref.mean((2, 3)))


@pytest.mark.parametrize('dtype', DTYPES)
def test_k25h_is_deterministic_graph_safe_and_stays_inside_y_and_the_mean(dtype, hip_lib):
    from metrabs_amd import kernels
    for (B, Cin, Cmid, H, W) in [(3, 40, 72, 8, 8), (2, 64, 256, 16, 16)]:
        x, w1, b1, wd, b2 = _inputs(B, Cin, Cmid, H, W, 5, dtype)
        a, am = kernels.expand_depthwise16(x, w1, b1, 'silu', wd, b2, 'silu', want_mean=True)
        a2, am2 = kernels.expand_depthwise16(x, w1, b1, 'silu', wd, b2, 'silu', want_mean=True)
        assert torch.equal(a, a2) and torch.equal(am, am2)
        for mapping in ('plain', 'xcd'):   # the bits do not depend on where a workgroup runs
            o, m = kernels.expand_depthwise16(x, w1, b1, 'silu', wd, b2, 'silu', want_mean=True, mapping=mapping)
            assert torch.equal(o, a) and torch.equal(m, am)
        # out= inside guard bands (64 elements either side: y's base stays 16-byte aligned)
        flat = torch.full((a.numel() + 128,), 7.0, device='cuda', dtype=dtype)
        out = flat[64:64 + a.numel()].view_as(a)
        assert kernels.expand_depthwise16(x, w1, b1, 'silu', wd, b2, 'silu', out=out) is out
        assert torch.equal(out, a)
        assert bool((flat[:64] == 7.0).all()) and bool((flat[-64:] == 7.0).all())
        # the mean inside guard bands, through the C entry
        mflat = torch.full((am.numel() + 128,), 7.0, device='cuda')
        wdf = wd.contiguous().float()
        rc = hip_lib.mtr_expand_dw16(
            ctypes.c_void_p(x.data_ptr()), 1 if dtype == torch.float16 else 2, ctypes.c_void_p(w1.data_ptr()),
            ctypes.c_void_p(b1.data_ptr()), 2, ctypes.c_void_p(wdf.data_ptr()), ctypes.c_void_p(b2.data_ptr()), 2,
            B, Cin, Cmid, H, W, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(mflat.data_ptr() + 64 * 4),
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(mflat[64:-64].view_as(am), am) and torch.equal(out, a)
        assert bool((mflat[:64] == 7.0).all()) and bool((mflat[-64:] == 7.0).all())
        assert bool((flat[:64] == 7.0).all()) and bool((flat[-64:] == 7.0).all())
        with torch.inference_mode():
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                kernels.expand_depthwise16(x, w1, b1, 'silu', wd, b2, 'silu', out=out)
                st.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                    kernels.expand_depthwise16(x, w1, b1, 'silu', wd, b2, 'silu', out=out)
            torch.cuda.current_stream().wait_stream(st)
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, a)
            assert bool((flat[:64] == 7.0).all()) and bool((flat[-64:] == 7.0).all())
        # a shifted, 16-byte-aligned base of x is accepted, one 8 bytes off is refused
        xflat = torch.zeros(x.numel() + 8, device='cuda', dtype=dtype)
        x8 = xflat[8:].view_as(x).copy_(x)
        assert kernels.expand_depthwise16_supported(x8, w1)
        assert torch.equal(kernels.expand_depthwise16(x8, w1, b1, 'silu', wd, b2, 'silu'), a)
        x4 = xflat[4:4 + x.numel()].view_as(x)
        assert not kernels.expand_depthwise16_supported(x4, w1)
        with pytest.raises(RuntimeError):
            kernels.expand_depthwise16(x4, w1, b1, 'silu', wd, b2, 'silu')


def test_k25h_wrapper_argument_checks(hip_lib):
    from metrabs_amd import kernels
    x, w1, b1, wd, b2 = _inputs(2, 8, 32, 8, 8, 1, torch.float16)
    ok, okm = kernels.expand_depthwise16(x, w1, b1, None, wd, b2, 'relu', want_mean=True)
    want, wmean = _chain(x, w1, b1, None, wd, b2, 'relu')
    assert torch.equal(ok, want) and torch.equal(okm, wmean)
    with pytest.raises(ValueError):
        kernels.expand_depthwise16(x, w1[:, :4].contiguous(), b1, None, wd, b2, None)      # W1 of another Cin
    with pytest.raises(ValueError):
        kernels.expand_depthwise16(x, w1.bfloat16(), b1, None, wd, b2, None)
    with pytest.raises(ValueError):
        kernels.expand_depthwise16(x, w1, b1, None, wd[:16], b2, None)                     # Wd of another Cmid
    with pytest.raises(ValueError):
        kernels.expand_depthwise16(x, w1, b1[:8], None, wd, b2, None)
    with pytest.raises(ValueError):
        kernels.expand_depthwise16(x.to(memory_format=torch.channels_last), w1, b1, None, wd, b2, None)
    with pytest.raises(ValueError):
        kernels.expand_depthwise16(x, w1, b1, None, wd, b2, None, out=torch.empty_like(ok).float())
    with pytest.raises(ValueError):
        kernels.expand_depthwise16(x, w1, b1, None, wd, b2, None, out=ok[:, :16])
    with pytest.raises(RuntimeError):   # MTR_E_SHAPE: no block-kernel plane
        kernels.expand_depthwise16(x.new_zeros(2, 8, 12, 12), w1, b1, None, wd, b2, None)
    with pytest.raises(RuntimeError):   # MTR_E_SHAPE: 1024 positions
        kernels.expand_depthwise16(x.new_zeros(1, 8, 32, 32), w1, b1, None, wd, b2, None)
    with pytest.raises((RuntimeError, TypeError)):
        kernels.expand_depthwise16(x.float(), w1.float(), b1, None, wd, b2, None)
    # y overlapping x: an expand of as many channels as its input, written in place
    xs, w1s, b1s, wds, b2s = _inputs(2, 8, 8, 8, 8, 2, torch.float16)
    with pytest.raises(RuntimeError):
        kernels.expand_depthwise16(xs, w1s, b1s, None, wds, b2s, None, out=xs)
    both = torch.zeros(2 * xs.numel(), device='cuda', dtype=torch.float16)
    xin = both[:xs.numel()].view_as(xs).copy_(xs)
    with pytest.raises(RuntimeError):   # a partial overlap, 16-byte aligned
        kernels.expand_depthwise16(xin, w1s, b1s, None, wds, b2s, None, out=both[64:64 + xs.numel()].view_as(xs))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        kernels.expand_depthwise16(x.cpu(), w1.cpu(), b1.cpu(), None, wd.cpu(), b2.cpu(), None)
    assert not kernels.expand_depthwise16_supported(x.to(memory_format=torch.channels_last), w1)
    assert not kernels.expand_depthwise16_supported(x.float(), w1)
    assert not kernels.expand_depthwise16_supported(x.new_zeros(2, 8, 12, 12), w1)
    assert kernels.expand_depthwise16_supported(x, w1)


# ---- the armed copies

def _calibrated(name, res, batch_size=4):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    return backbones.calibrate_batchnorm(backbones.build_backbone(name).cuda(), res, 'cuda', batch_size=batch_size)


def _paths(net):
    return [(type(m).__name__, getattr(m, 'last_path', None)) for m in net.modules()]


def _pairs(net):
    from metrabs_amd import backbones
    return [(m, m.hand_to[0]) for m in net.modules() if isinstance(m, backbones.ConvBiasAct) and m.hand_to]


@pytest.fixture(scope='module')
def nets():
    return {name: _calibrated(name, 256) for name in ('efficientnetv2-s', 'mobilenetv3')}


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['efficientnetv2-s', 'mobilenetv3'])
def test_armed_copy_takes_k25h_where_it_applies_and_keeps_the_bits(name, dtype, nets, hip_lib):
    from metrabs_amd import backbones
    DW = backbones.DepthwiseBiasAct
    net = nets[name]
    plain = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, fuse_expand_depthwise=True)
    assert not _pairs(plain)
    assert list(plain.state_dict()) == list(armed.state_dict())
    assert [type(m) for m in plain.modules()] == [type(m) for m in armed.modules()]
    pairs = _pairs(armed)
    assert len(pairs) == {'efficientnetv2-s': 28, 'mobilenetv3': 6}[name]
    x = torch.rand(2, 3, 256, 256, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    seen = {}
    hs = [e.register_forward_pre_hook(lambda mod, args: seen.__setitem__(mod, tuple(args[0].shape))) for e, _ in pairs]
    shipped = DW.k25h_slower
    try:
        with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
            off = plain(x)
            # as shipped: the classes of k25h_slower keep the chain, the others fuse; the same bits
            assert torch.equal(armed(x), off)
            key = lambda e: (seen[e][1], e.conv.out_channels, seen[e][2], seen[e][3])
            for e, d in pairs:
                fused = seen[e][2] * seen[e][3] <= 256 and key(e) not in shipped
                assert (e.last_path == 'k25h') == fused == (d.last_path == 'k25h'), (key(e), e.last_path, d.last_path)
            assert any(e.last_path == 'k25h' for e, _ in pairs)
            # the list emptied: every pair the kernel takes runs on it
            DW.k25h_slower = frozenset()
            on = armed(x)
            assert torch.equal(on, off)
            took = 0
            for e, d in pairs:
                B, K, H, W = seen[e]
                fits = H * W <= 256 and (K, e.conv.out_channels, H * W) not in backbones.ConvBiasAct.k13h_slower \
                    and (K, e.conv.out_channels, H, W) not in DW.k25h_slower
                if fits:
                    assert (e.last_path, d.last_path) == ('k25h', 'k25h'), (seen[e], e.last_path, d.last_path)
                else:
                    assert e.last_path != 'k25h' and d.last_path == 'k11', (seen[e], e.last_path, d.last_path)
                took += fits
            # -S: every stride-1 MBConv block (16x16 and 8x8); MobileNetV3: the five 16x16 blocks, not the 64x64 one
            assert took == {'efficientnetv2-s': 28, 'mobilenetv3': 5}[name]
            # every other layer reports what it reports in the default copy (stride 2, 5x5, 64x64, the projects, ...)
            fused = {id(m) for p in pairs if p[0].last_path == 'k25h' for m in p}
            rest_on = [(type(m).__name__, getattr(m, 'last_path', None)) for m in armed.modules() if id(m) not in fused]
            rest_off = [(type(m).__name__, getattr(m, 'last_path', None)) for m, a in zip(plain.modules(), armed.modules())
                        if id(a) not in fused]
            assert rest_on == rest_off
            # the class switch, and a filled k25h_slower, send every pair back to the chain
            DW.use_k25h = False
            assert torch.equal(armed(x), off) and _paths(armed) == _paths(plain)
            DW.use_k25h = True
            DW.k25h_slower = frozenset(key(e) for e, _ in pairs)
            assert torch.equal(armed(x), off) and _paths(armed) == _paths(plain)
            DW.k25h_slower = frozenset()
            # both restored: the pairs fuse again
            assert torch.equal(armed(x), off)
            assert sum(e.last_path == 'k25h' for e, _ in pairs) == took
    finally:
        DW.use_k25h = True
        DW.k25h_slower = shipped
        for h in hs:
            h.remove()
    assert on.dtype == dtype and torch.isfinite(on).all()


@pytest.mark.parametrize('dtype', DTYPES)
def test_k25h_with_the_other_options(dtype, nets, hip_lib):
    """fuse_blocks, fuse_stem, block_depthwise and deep_projects touch other modules: the copy with all of them and
    fuse_expand_depthwise has the bits of the copy with them alone (deep_projects itself differs from the default
    copy by rounding), and the pairs still run K25h."""
    from metrabs_amd import backbones
    others = dict(fuse_blocks=True, fuse_stem=True, block_depthwise=True, deep_projects=True)
    net = nets['efficientnetv2-s']
    base = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, **others)
    both = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, fuse_expand_depthwise=True, **others)
    x = torch.rand(2, 3, 256, 256, device='cuda', generator=torch.Generator(device='cuda').manual_seed(2))
    DW = backbones.DepthwiseBiasAct
    shipped, DW.k25h_slower = DW.k25h_slower, frozenset()   # every pair the kernel takes
    try:
        with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
            assert torch.equal(both(x), base(x))
    finally:
        DW.k25h_slower = shipped
    pairs = _pairs(both)
    assert len(pairs) == 28 and sum(e.last_path == 'k25h' and d.last_path == 'k25h' for e, d in pairs) == 28
    fused = {id(m) for p in pairs if p[0].last_path == 'k25h' for m in p}
    assert [getattr(a, 'last_path', None) for a in both.modules() if id(a) not in fused] == \
        [getattr(m, 'last_path', None) for m, a in zip(base.modules(), both.modules()) if id(a) not in fused]


def test_a_refusal_after_the_hand_over_still_runs_the_expand(nets, hip_lib):
    """Whatever changes between the expand's question and the depthwise layer's forward: a tensor never skips its
    expand."""
    from metrabs_amd import backbones
    DW = backbones.DepthwiseBiasAct
    armed = backbones.fold_batchnorm(nets['efficientnetv2-s'], fused_epilogue=True, dtype=torch.float16,
                                     fuse_expand_depthwise=True)
    e, d = _pairs(armed)[0]
    x = torch.randn(2, e.conv.in_channels, 16, 16, device='cuda').half()
    try:
        with torch.inference_mode():
            want = d(e.forward_here(x))
            assert e(x) is x and e.last_path == 'k25h'
            DW.use_k25h = False
            got = d(x)
            assert torch.equal(got, want) and d.last_path == 'k11' and e.last_path == 'k13h'
            DW.use_k25h = True
            assert e(x) is x
            fused = d(x)
            assert torch.equal(fused, want) and d.last_path == 'k25h'
            # a tensor that was NOT handed over is an ordinary input of the depthwise layer
            assert e(x) is x
            other = want.clone()
            assert torch.equal(d(other), d.forward(other)) and d.last_path == 'k11'
    finally:
        DW.use_k25h = True


def _model_dir(tmp_path):
    from metrabs_amd import backbones, loading
    from metrabs_amd.config import MetrabsConfig
    from metrabs_amd.joint_info import JointInfo
    from metrabs_amd.models.metrabs import Metrabs
    raw = dict(proc_side=256, stride_train=32, stride_test=32, centered_stride=True, depth=8,
               box_size_mm=2200, efficientnet_size='s', weak_perspective=False, mix_3d_inside_fov=0.5)
    bb = backbones.efficientnetv2('s')
    model = Metrabs(bb, JointInfo(cases.COCO17, cases.COCO17_EDGES), MetrabsConfig.from_any(raw),
                    in_channels=bb.out_channels)
    model.load_state_dict(cases.deterministic_state(model.state_dict(), seed=11))
    skel = {'': dict(indices=list(range(17)), names=cases.COCO17, edges=cases.COCO17_EDGES)}
    d = str(tmp_path / 'model')
    loading.save_model_dir(d, model, raw, skel, np.eye(17, dtype=np.float32))
    return d


def _poses(est, images, boxes):
    with torch.inference_mode():
        r = est.estimate_poses_batched(images, boxes, num_aug=2)
    return torch.cat(r['poses3d']).clone()


def test_k25h_through_the_loader_and_the_api(tmp_path, hip_lib):
    from metrabs_amd import loading
    d = _model_dir(tmp_path)
    with pytest.raises(ValueError):
        loading.load_crop_model(d, fuse_expand_depthwise=True)
    with pytest.raises(ValueError):
        loading.load_multiperson_model(d, fuse_expand_depthwise=True)
    plain = loading.load_multiperson_model(d, dtype=torch.float16)
    plain.crop_model.deterministic_backbone = True
    plain.graph_batches = False
    est = loading.load_multiperson_model(d, dtype=torch.float16, fuse_expand_depthwise=True)
    est.crop_model.deterministic_backbone = True
    est.graph_batches = True
    eager = loading.load_multiperson_model(d, dtype=torch.float16, fuse_expand_depthwise=True)
    eager.crop_model.deterministic_backbone = True
    eager.graph_batches = False
    for seed in (5, 9):
        images = torch.stack([cases.synth_images(1, 240, 320, seed + i)[0] for i in range(2)]).cuda()
        boxes = [torch.tensor([[60.0, 20.0, 120.0, 200.0], [150.0, 30.0, 100.0, 180.0]]),
                 torch.tensor([[40.0, 10.0, 140.0, 210.0]])]
        ref, a, b = _poses(plain, images, boxes), _poses(eager, images, boxes), _poses(est, images, boxes)
        assert torch.isfinite(a).all()
        assert torch.equal(a, ref), float((a - ref).abs().max())   # the armed copy returns the unarmed copy's bits
        assert torch.equal(a, b), float((a - b).abs().max())       # a graphed call returns the eager call's bits
    for model in (est, eager):
        pairs = _pairs(model.crop_model.backbone)
        assert len(pairs) == 28 and any(e.last_path == 'k25h' and dw.last_path == 'k25h' for e, dw in pairs)
    assert not _pairs(plain.crop_model.backbone)
    assert est.graphs.stats['captures'] >= 1 and est.graphs.stats['replays'] >= 1, est.graphs.stats

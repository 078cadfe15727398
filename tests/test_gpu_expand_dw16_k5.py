"""GPU: K28h (csrc/expand_dw16_k5.hip) -- the 1x1 expand of an MBConv block of the 16-bit inference copy (K13h) and the
depthwise 5x5 layer behind it (K15), stride 1 or 2, padding 2, with the squeeze-excite mean, as one launch.

The kernel's contract is BITS: y and the mean torch.equal to kernels.conv1x1_bias_act16 followed by
kernels.depthwise5x5_bias_act(.., stride, 2, want_mean=True) on the same tensors.  One check does not rest on the chain:
small integers, where every partial sum is exact in 16 bits, against an integer convolution computed in fp64.

The shapes are the smallest at which each part of the kernel can go wrong (SHAPES says which).  Then every activation
pair, the mean on and off, the mappings, a second call, a graph replay, out= inside guard bands, the wrapper's refusals;
the armed copies of MobileNetV3 at 128 px and 256 px (paths, the switch, the slower list, the other options beside it);
the loader and the API on a MobileNetV3 model."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cases
from test_expand_dw16_k5_host import lds_rule
from test_gpu_expand_dw16 import ACTS, DTYPES, _act64, _calibrated, _paths, _poses

pytestmark = pytest.mark.gpu

# the largest plane with more than 64 units (so a lane sums more than one unit sum) that the LDS rule admits: 40x40, 100
# units, is refused at 32 channels
BIG = max(((H * W, H, W) for H in range(1, 113) for W in range(1, 113)
           if lds_rule(8, H, W, 1) and -(-H // 4) * (W // 4) > 64))[1:]

# (B, Cin, Cmid, H, W, stride)
SHAPES = [
    (3, 8, 40, 8, 8, 1),       # a partial channel tile; B no multiple of 8 under the xcd mapping
    (1, 24, 72, 16, 16, 2),    # a k tail below one 32-k tile; OH x OW = 8x8, units = 8
    (2, 72, 33, 32, 32, 1),    # several k-tiles and a tail; 1024 positions: phase 1 in four passes; units = 64 = G; one
                               # live channel in the last 32-row tile
    (1, 16, 32, 12, 16, 1),    # UH RB > OH: the row_ok rows; rectangular
    (1, 16, 8) + BIG + (1,),   # more than 64 units: a lane sums two unit sums; the last pass is partial
    (2, 8, 64, 4, 4, 1),       # 16 positions: one tile, its rows past HW zero
    (2, 16, 72, 8, 8, 2),      # 64 channels a workgroup and a second, partial one; 4x4 outputs, two units
]


def _inputs(B, Cin, Cmid, H, W, seed, dtype, border=8.0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(B, Cin, H, W, device='cuda', generator=g)
    edge = torch.ones(H, W, device='cuda')   # large border pixels: a wrong halo or padding element shows
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = border
    x = (x * edge).to(dtype)
    w1 = (torch.randn(Cmid, Cin, device='cuda', generator=g) / Cin ** 0.5).to(dtype)
    b1 = 0.5 * torch.randn(Cmid, device='cuda', generator=g)
    wd = torch.randn(Cmid, 1, 5, 5, device='cuda', generator=g) * 0.25
    b2 = torch.randn(Cmid, device='cuda', generator=g)
    return x, w1, b1, wd, b2


def _chain(x, w1, b1, act1, wd, b2, act2, stride):
    from metrabs_amd import kernels
    mid = kernels.conv1x1_bias_act16(x, w1, b1, act1)
    return kernels.depthwise5x5_bias_act(mid, wd, b2, act2, stride, 2, want_mean=True)


def _same(got, want, label):
    assert got.shape == want.shape and got.dtype == want.dtype, label
    assert torch.equal(got, want), (label, int((got != want).sum()), float((got.float() - want.float()).abs().max()))


def test_the_largest_plane_with_more_than_64_units(hip_lib):
    """BIG comes from the restated rule; the C query agrees: 28x52 takes all 160 KiB, 40x40 is refused."""
    q = hip_lib.mtr_expand_dw16_k5_lds_bytes
    assert BIG == (28, 52) and q(1, 16, 8, *BIG, 1) == lds_rule(8, *BIG, 1) == 160 * 1024
    assert q(1, 16, 8, 40, 40, 1) == lds_rule(8, 40, 40, 1) == 0


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', SHAPES, ids=lambda c: '{}-{}-{}-{}x{}-s{}'.format(*c))
def test_k28h_has_the_chains_bits(case, dtype, hip_lib):
    from metrabs_amd import kernels
    B, Cin, Cmid, H, W, stride = case
    x, w1, b1, wd, b2 = _inputs(B, Cin, Cmid, H, W, 100 + Cin + H, dtype)
    assert kernels.expand_depthwise16_k5_supported(x, w1, stride), case
    assert kernels.conv1x1_16_supported(x, w1) and kernels.depthwise5x5_supported(H, W, 2)
    want, want_mean = _chain(x, w1, b1, 'hardswish', wd, b2, 'hardswish', stride)
    got, mean = kernels.expand_depthwise16_k5(x, w1, b1, 'hardswish', wd, b2, 'hardswish', stride, want_mean=True)
    assert got.shape == (B, Cmid, (H - 1) // stride + 1, (W - 1) // stride + 1)
    assert mean.shape == (B, Cmid) and mean.dtype == torch.float32
    _same(got, want, case)
    _same(mean, want_mean, case)
    # without the mean: the same y, one tensor
    alone = kernels.expand_depthwise16_k5(x, w1, b1, 'hardswish', wd, b2, 'hardswish', stride)
    assert isinstance(alone, torch.Tensor)
    _same(alone, want, case)
    # the 4-d and 3-d forms of the weights
    again = kernels.expand_depthwise16_k5(x, w1[:, :, None, None], b1, 'hardswish', wd[:, 0], b2, 'hardswish', stride)
    _same(again, want, case)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('stride', [1, 2])
def test_k28h_every_activation_pair(stride, dtype, hip_lib):
    from metrabs_amd import kernels
    x, w1, b1, wd, b2 = _inputs(2, 24, 40, 12, 16, 11, dtype)
    for act1 in ACTS:
        for act2 in ACTS:
            want, want_mean = _chain(x, w1, b1, act1, wd, b2, act2, stride)
            got, mean = kernels.expand_depthwise16_k5(x, w1, b1, act1, wd, b2, act2, stride, want_mean=True)
            _same(got, want, (act1, act2))
            _same(mean, want_mean, (act1, act2))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('act', [None, 'relu'])
@pytest.mark.parametrize('stride', [1, 2])
def test_k28h_is_exact_on_small_integers(stride, act, dtype, hip_lib):
    """Small-integer data, an expand that looks at two input channels per output channel and an asymmetric depthwise
    weight: every product, every partial sum, the intermediate and the output are integers of at most 2^8 in magnitude
    (exact in bf16, hence in f16), checked here on the reference -- so the result must EQUAL the integer evaluation in
    fp64, whatever the chain says: a swapped tap, a transposed fragment, a wrong pass, chunk or ring element cannot hide
    in rounding.  The plane has a power-of-two number of outputs, so the mean is exact as well."""
    from metrabs_amd import kernels
    Cin, Cmid, H, W = 24, 72, 16, 16
    g = torch.Generator(device='cuda').manual_seed(3)
    x = torch.randint(-1, 2, (2, Cin, H, W), device='cuda', generator=g).float()
    c = torch.arange(Cmid, device='cuda')
    w1 = torch.zeros(Cmid, Cin, device='cuda')
    w1[c, c % Cin] = torch.where(c % 2 == 0, 1.0, -1.0)
    w1[c, (5 * c + 7) % Cin] += torch.where(c % 3 == 0, 2.0, -1.0)
    b1 = c.float() % 3 - 1
    taps = ((torch.arange(25, device='cuda') * 7) % 5 - 2).float()   # -2 .. 2, five of each, no symmetry
    wd = torch.stack([torch.roll(taps, int(i)) for i in range(25)])[c % 25].view(Cmid, 1, 5, 5) \
        * torch.where(c % 2 == 0, 1.0, -1.0).view(-1, 1, 1, 1)
    b2 = torch.zeros(Cmid, device='cuda') if act is None else c.float() % 7 - 3
    mid = _act64(F.conv2d(x.double(), w1.double()[:, :, None, None], b1.double()), act)
    ref = _act64(F.conv2d(mid, wd.double(), b2.double(), stride, 2, groups=Cmid), act)
    assert float(mid.abs().max()) <= 5 and float(ref.abs().max()) <= 30 * 5 + 3 <= 2 ** 8
    assert float(ref.abs().max()) > 10   # (more than one tap can give: not a trivially small case)
    got, mean = kernels.expand_depthwise16_k5(x.to(dtype), w1.to(dtype), b1, act, wd, b2, act, stride, want_mean=True)
    assert torch.equal(got.double(), ref)
    assert torch.equal(mean.double(), ref.mean((2, 3)))
    # zero biases in front of the expand too: the issue's plain integer convolution
    z = torch.zeros(Cmid, device='cuda')
    mid0 = F.conv2d(x.double(), w1.double()[:, :, None, None])
    ref0 = F.conv2d(mid0, wd.double(), None, stride, 2, groups=Cmid)
    assert float(ref0.abs().max()) <= 2 ** 8
    got0 = kernels.expand_depthwise16_k5(x.to(dtype), w1.to(dtype), z, None, wd, z, None, stride)
    assert torch.equal(got0.double(), ref0)


@pytest.mark.parametrize('dtype', DTYPES)
def test_k28h_is_deterministic_graph_safe_and_stays_inside_y(dtype, hip_lib):
    from metrabs_amd import kernels
    fn = kernels.expand_depthwise16_k5
    # B = 9: under the xcd mapping the grid is padded to 16 images, and workgroups past the batch leave at once
    for (B, Cin, Cmid, H, W, stride) in [(9, 16, 40, 8, 8, 1), (2, 24, 72, 16, 16, 2), (2, 40, 33, 32, 32, 1)]:
        x, w1, b1, wd, b2 = _inputs(B, Cin, Cmid, H, W, 5, dtype)
        args = (x, w1, b1, 'silu', wd, b2, 'relu', stride)
        a, am = fn(*args, want_mean=True)
        want, want_mean = _chain(*args)
        _same(a, want, (B, H, W))
        _same(am, want_mean, (B, H, W))
        for mapping in ('plain', 'xcd', 'auto'):
            b, bm = fn(*args, want_mean=True, mapping=mapping)
            assert torch.equal(a, b) and torch.equal(am, bm), mapping
        # out= inside guard bands (64 elements either side: y's base stays 16-byte aligned)
        flat = torch.full((a.numel() + 128,), 7.0, device='cuda', dtype=dtype)
        out = flat[64:64 + a.numel()].view_as(a)
        got = fn(*args, want_mean=True, out=out)
        assert got[0] is out and torch.equal(out, a) and torch.equal(got[1], am)
        assert bool((flat[:64] == 7.0).all()) and bool((flat[-64:] == 7.0).all())
        with torch.inference_mode():
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                fn(*args, out=out)
                st.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                    _, gm = fn(*args, want_mean=True, out=out)
            torch.cuda.current_stream().wait_stream(st)
            for _ in range(2):
                out.zero_()
                gm.zero_()
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, a) and torch.equal(gm, am)
            assert bool((flat[:64] == 7.0).all()) and bool((flat[-64:] == 7.0).all())
        # a shifted, 16-byte-aligned base of x is accepted, one 8 bytes off is refused
        xflat = torch.zeros(x.numel() + 8, device='cuda', dtype=dtype)
        x8 = xflat[8:].view_as(x).copy_(x)
        assert kernels.expand_depthwise16_k5_supported(x8, w1, stride)
        assert torch.equal(fn(x8, *args[1:]), a)
        x4 = xflat[4:4 + x.numel()].view_as(x)
        assert not kernels.expand_depthwise16_k5_supported(x4, w1, stride)
        with pytest.raises(RuntimeError):
            fn(x4, *args[1:])


def test_k28h_wrapper_argument_checks(hip_lib):
    from metrabs_amd import kernels
    fn, ask = kernels.expand_depthwise16_k5, kernels.expand_depthwise16_k5_supported
    x, w1, b1, wd, b2 = _inputs(2, 16, 24, 8, 8, 1, torch.float16)
    ok = fn(x, w1, b1, 'relu', wd, b2, 'relu')
    with pytest.raises(ValueError, match='NCHW-contiguous'):
        fn(x.to(memory_format=torch.channels_last), w1, b1, None, wd, b2, None)
    with pytest.raises(ValueError, match='stride must be 1 or 2'):
        fn(x, w1, b1, None, wd, b2, None, stride=3)
    with pytest.raises(ValueError, match='input channels'):
        fn(x, w1[:, :8].contiguous(), b1, None, wd, b2, None)
    with pytest.raises(ValueError, match='the 1x1 weight is'):
        fn(x, w1.bfloat16(), b1, None, wd, b2, None)
    with pytest.raises(ValueError, match=r'the depthwise weight must be \[24, 5, 5\]'):
        fn(x, w1, b1, None, wd[:, :, :3, :3].contiguous(), b2, None)
    with pytest.raises(ValueError, match='biases'):
        fn(x, w1, b1[:8], None, wd, b2, None)
    with pytest.raises(KeyError):
        fn(x, w1, b1, None, wd, b2, None, mapping='other')
    with pytest.raises(ValueError):
        fn(x, w1, b1, None, wd, b2, None, out=torch.empty(2, 24, 4, 4, device='cuda', dtype=torch.float16))
    with pytest.raises(RuntimeError):   # the entry's own refusal: a plane whose slice does not fit
        fn(x.new_zeros(1, 16, 64, 64), w1, b1, None, wd, b2, None, stride=2)
    with pytest.raises(RuntimeError):   # f32 is refused by the entry (MTR_E_DTYPE)
        fn(x.float(), w1.float(), b1, None, wd, b2, None)
    assert ask(x, w1) and ask(x, w1, 2) and ask(x, w1[:, :, None, None])
    assert not ask(x.float(), w1.float()) and not ask(x, w1.bfloat16())
    assert not ask(x.new_zeros(1, 16, 64, 64), w1, 2) and not ask(x.new_zeros(1, 16, 6, 6), w1)
    assert not ask(x.new_zeros(1, 12, 8, 8), w1[:, :12].contiguous())
    assert torch.equal(ok, fn(x, w1, b1, 'relu', wd, b2, 'relu'))


# ---- the armed copies

FIELD = 'hand_k5_to'
# (Cin, Cmid, H, W, stride) of the six pairs' expand inputs at 128 px and at 256 px
AT_128 = [(24, 72, 32, 32, 2), (40, 120, 16, 16, 1), (40, 120, 16, 16, 1), (112, 672, 8, 8, 2), (160, 960, 4, 4, 1),
          (160, 960, 4, 4, 1)]
AT_256 = [(K, M, 2 * H, 2 * W, s) for K, M, H, W, s in AT_128]


def _pairs(net, field=FIELD):
    from metrabs_amd import backbones
    return [(m, getattr(m, field)[0]) for m in net.modules()
            if isinstance(m, backbones.ConvBiasAct) and getattr(m, field)]


@pytest.fixture(scope='module')
def net():
    return _calibrated('mobilenetv3', 128)


def _x(B, res, seed):
    return torch.rand(B, 3, res, res, device='cuda', generator=torch.Generator(device='cuda').manual_seed(seed))


def _run(net, x):
    with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        return net(x)


def _watch(pairs):
    seen = {}
    hooks = [e.register_forward_pre_hook(lambda mod, args: seen.__setitem__(mod, tuple(args[0].shape)))
             for e, _ in pairs]
    return seen, hooks


def _key(seen, e, d):
    return (seen[e][1], e.conv.out_channels, seen[e][2], seen[e][3], d.stride)


def test_armed_mobilenetv3_takes_k28h_on_all_six_pairs_at_128_px(net, hip_lib):
    from metrabs_amd import backbones
    DW = backbones.DepthwiseBiasAct
    plain = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=torch.float16)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=torch.float16, fuse_expand_depthwise5x5=True)
    assert not _pairs(plain) and list(plain.state_dict()) == list(armed.state_dict())
    assert not any(_pairs(armed, f) for f in ('hand_to', 'hand_planes_to', 'hand_tiles_to'))
    pairs = _pairs(armed)
    assert len(pairs) == 6
    x = _x(2, 128, 1)
    seen, hs = _watch(pairs)
    shipped, DW.k28h_slower = DW.k28h_slower, frozenset()
    try:
        off = _run(plain, x)
        on = _run(armed, x)
        assert torch.equal(on, off)
        assert [_key(seen, e, d) for e, d in pairs] == AT_128
        for e, d in pairs:
            with torch.inference_mode():
                asked = e.path(torch.empty(seen[e], device='cuda', dtype=torch.float16))
            assert (e.last_path, d.last_path, asked) == ('k28h', 'k28h', 'k28h'), _key(seen, e, d)
        # every other layer reports what it reports in the default copy
        fused = {id(m) for p in pairs for m in p}
        assert [(type(a).__name__, getattr(a, 'last_path', None)) for a in armed.modules() if id(a) not in fused] == \
            [(type(m).__name__, getattr(m, 'last_path', None)) for m, a in zip(plain.modules(), armed.modules())
             if id(a) not in fused]
        twin = {id(a): m for m, a in zip(plain.modules(), armed.modules())}
        assert {(twin[id(e)].last_path, twin[id(d)].last_path) for e, d in pairs} == {('k13h', 'k15')}
        # the class switch, and a shape put into k28h_slower, send the pairs back to the chain
        DW.use_k28h = False
        assert torch.equal(_run(armed, x), off) and _paths(armed) == _paths(plain)
        DW.use_k28h = True
        DW.k28h_slower = frozenset({AT_128[1], AT_128[3]})
        assert torch.equal(_run(armed, x), off)
        for e, d in pairs:
            want = ('k13h', 'k15') if _key(seen, e, d) in DW.k28h_slower else ('k28h', 'k28h')
            assert (e.last_path, d.last_path) == want, _key(seen, e, d)
        # as shipped: the listed shapes keep the chain, the others fuse; the same bits
        DW.k28h_slower = shipped
        assert torch.equal(_run(armed, x), off)
        for e, d in pairs:
            want = ('k13h', 'k15') if _key(seen, e, d) in shipped else ('k28h', 'k28h')
            assert (e.last_path, d.last_path) == want, _key(seen, e, d)
    finally:
        DW.use_k28h = True
        DW.k28h_slower = shipped
        for h in hs:
            h.remove()
    assert on.dtype == torch.float16 and torch.isfinite(on).all()


@pytest.mark.parametrize('dtype', DTYPES)
def test_armed_mobilenetv3_at_256_px_fuses_what_the_query_accepts(dtype, net, hip_lib):
    from metrabs_amd import backbones, kernels
    DW = backbones.DepthwiseBiasAct
    plain = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, fuse_expand_depthwise5x5=True)
    pairs = _pairs(armed)
    x = _x(1, 256, 2)
    seen, hs = _watch(pairs)
    shipped, DW.k28h_slower = DW.k28h_slower, frozenset()
    try:
        off = _run(plain, x)
        assert torch.equal(_run(armed, x), off)
        assert [_key(seen, e, d) for e, d in pairs] == AT_256
        taken = 0
        for e, d in pairs:
            K, M, H, W, s = _key(seen, e, d)
            accepts = kernels._lib.load().mtr_expand_dw16_k5_lds_bytes(1, K, M, H, W, s) > 0
            assert accepts == ((H, W, s) != (64, 64, 2))
            want = ('k28h', 'k28h') if accepts else ('k13h', 'k15')
            assert (e.last_path, d.last_path) == want, (K, M, H, W, s)
            taken += accepts
        assert taken == 5
    finally:
        DW.k28h_slower = shipped
        for h in hs:
            h.remove()


def test_k28h_beside_the_other_expand_depthwise_options_and_block_depthwise(net, hip_lib):
    """fuse_expand_depthwise (K25h), fuse_expand_depthwise_tiles (K27h) and block_depthwise (K18) beside the new option:
    separate fields, disjoint layers (k = 3 against k = 5).  Every pair reports the path its own option gives alone, and
    the features are the default copy's."""
    from metrabs_amd import backbones
    DW = backbones.DepthwiseBiasAct
    dtype = torch.float16
    fold = lambda **kw: backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, **kw)
    plain = fold()
    others = fold(fuse_expand_depthwise=True, fuse_expand_depthwise_tiles=True, block_depthwise=True)
    all4 = fold(fuse_expand_depthwise=True, fuse_expand_depthwise_tiles=True, block_depthwise=True,
                fuse_expand_depthwise5x5=True)
    pairs = _pairs(all4)
    assert len(pairs) == 6 and len(_pairs(all4, 'hand_to')) == 6 and len(_pairs(all4, 'hand_tiles_to')) == 8
    x = _x(2, 128, 3)
    shipped, DW.k28h_slower = DW.k28h_slower, frozenset()
    try:
        off = _run(plain, x)
        assert torch.equal(_run(others, x), off)
        assert torch.equal(_run(all4, x), off)
        assert all((e.last_path, d.last_path) == ('k28h', 'k28h') for e, d in pairs)
        # everything but the six pairs reports what the copy without the new option reports
        fused = {id(m) for p in pairs for m in p}
        assert [(type(a).__name__, a.last_path) for a in all4.modules() if hasattr(a, 'last_path') and
                id(a) not in fused] == \
            [(type(m).__name__, m.last_path) for m, a in zip(others.modules(), all4.modules())
             if hasattr(a, 'last_path') and id(a) not in fused]
        assert any(getattr(m, 'last_path', None) in ('k25h', 'k27h') for m in all4.modules())
    finally:
        DW.k28h_slower = shipped


def test_a_refusal_after_the_hand_over_still_runs_the_expand(net, hip_lib):
    """Whatever changes between the expand's question and the depthwise layer's forward: a tensor never skips its
    expand."""
    from metrabs_amd import backbones
    DW = backbones.DepthwiseBiasAct
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=torch.float16, fuse_expand_depthwise5x5=True)
    shipped, DW.k28h_slower = DW.k28h_slower, frozenset()
    try:
        e, d = _pairs(armed)[3]   # 112 -> 672, stride 2, with the mean
        x = torch.randn(2, 112, 8, 8, device='cuda').half()
        with torch.inference_mode():
            want = d(e.forward_here(x))
            want_mean = d.take_mean_f32(want)
            assert want_mean is not None
            assert e.hands_over(x) and e(x) is x and e.last_path == 'k28h'
            DW.use_k28h = False
            got = d(x)
            assert torch.equal(got, want) and d.last_path == 'k15' and e.last_path == 'k13h'
            DW.use_k28h = True
            assert e(x) is x
            fused = d(x)
            assert torch.equal(fused, want) and d.last_path == 'k28h'
            assert torch.equal(d.take_mean_f32(fused), want_mean)
            # a tensor that was NOT handed over is an ordinary input of the depthwise layer
            assert e(x) is x
            other = e.forward_here(x).clone()
            assert torch.equal(d(other), want) and d.last_path == 'k15'
    finally:
        DW.use_k28h = True
        DW.k28h_slower = shipped


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


def test_k28h_through_the_loader_and_the_api(tmp_path, hip_lib):
    from metrabs_amd import backbones, loading
    DW = backbones.DepthwiseBiasAct
    d = _model_dir(tmp_path, _calibrated('mobilenetv3', 256).cpu())
    with pytest.raises(ValueError):
        loading.load_crop_model(d, fuse_expand_depthwise5x5=True)
    with pytest.raises(ValueError):
        loading.load_multiperson_model(d, fuse_expand_depthwise5x5=True)
    plain = loading.load_multiperson_model(d, dtype=torch.float16)
    plain.crop_model.deterministic_backbone = True
    plain.graph_batches = False
    est = loading.load_multiperson_model(d, dtype=torch.float16, fuse_expand_depthwise5x5=True)
    est.crop_model.deterministic_backbone = True
    est.graph_batches = True
    eager = loading.load_multiperson_model(d, dtype=torch.float16, fuse_expand_depthwise5x5=True)
    eager.crop_model.deterministic_backbone = True
    eager.graph_batches = False
    shipped, DW.k28h_slower = DW.k28h_slower, frozenset()
    try:
        images = torch.stack([cases.synth_images(1, 240, 320, 5 + i)[0] for i in range(2)]).cuda()
        boxes = [torch.tensor([[60.0, 20.0, 120.0, 200.0], [150.0, 30.0, 100.0, 180.0]]),
                 torch.tensor([[40.0, 10.0, 140.0, 210.0]])]
        ref, a, b = _poses(plain, images, boxes), _poses(eager, images, boxes), _poses(est, images, boxes)
        assert torch.isfinite(a).all()
        assert torch.equal(a, ref), float((a - ref).abs().max())   # the armed copy returns the unarmed copy's bits
        assert torch.equal(a, b), float((a - b).abs().max())       # a graphed call returns the eager call's bits
    finally:
        DW.k28h_slower = shipped
    for model in (est, eager):
        pairs = _pairs(model.crop_model.backbone)
        assert len(pairs) == 6
        assert sum(e.last_path == 'k28h' and dw.last_path == 'k28h' for e, dw in pairs) == 5   # (64x64 keeps the chain)
    assert not _pairs(plain.crop_model.backbone)

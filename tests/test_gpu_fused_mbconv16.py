"""GPU: K16h (csrc/fused_mbconv16.hip), a FusedMBConv block of the 16-bit inference copy -- the 3x3 expand of K14h and
the 1x1 project of K13h -- as one launch with the intermediate in LDS.

Three independent checks per shape.  (1) BITS: torch.equal to kernels.conv3x3_bias_act16 followed by
kernels.conv1x1_bias_act16 on the same tensors -- the kernel's contract.  (2) fp64, independently of the chain: the
whole block in float64 on the 16-bit operands, the intermediate NOT rounded.  (3) small integers, exact.

The fp64 bound, in the manner of test_gpu_conv3x3_16._check (section 12's form) carried through the block.  With
z3 = conv3x3(x, W3) + b3, s3 = conv3x3(|x|, |W3|) + |b3|, m = act(z3), u(v) = one unit in the last place of the
16-bit format at |v|:

    d_mid = u(m) + L * 9 Cin * 2^-24 * s3 + 1e-6 |m| + 2^-24
            (K14h's bound: f32 accumulation over K = 9 Cin through an activation of Lipschitz constant L -- 1 for none
            and relu, 1.1 for silu, 1.5 for hardswish -- then ONE 16-bit rounding of the intermediate)
    s1    = sum_c |W1[m, c]| (|m_c| + d_mid_c) + |b1|
    bound = sum_c |W1[m, c]| d_mid_c                      (the intermediate's error carried through the project)
            + 1.1 * Cmid * 2^-24 * s1                      (the project's own f32 accumulation, K = Cmid)
            + 2^-23 (s1 + |residual|)                      (the two f32 additions of the epilogue)
            + 1e-6 |ref| + 2^-24 + u(ref)                  (one output rounding)

Every element is checked; the largest error as a share of the bound is printed (DESIGN.md section 16 records it).
Then: determinism, out=, graph replay, guard bands, alignment, the argument rules, the shape query; the armed copy of
every backbone (paths, fallbacks, the untouched default copy, accuracy against the f32 network); the loader and the
API."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cases

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
ACTS = [None, 'relu', 'silu', 'hardswish']
_TORCH_ACT = {None: lambda t: t, 'relu': F.relu, 'silu': F.silu, 'hardswish': F.hardswish}
_MANT = {torch.float16: 10, torch.bfloat16: 7}
_LIPSCHITZ = {None: 1.0, 'relu': 1.0, 'silu': 1.1, 'hardswish': 1.5}

# (Cin, Cmid, Cout, stride, H, W, skip): the smallest shapes at which each mechanism can go wrong; Ho Wo % 8 == 0
SHAPES = [
    (24, 96, 48, 2, 16, 16, False),    # 9 Cin / 8 odd (a half step); a single chunk of Cmid
    (48, 192, 48, 1, 16, 16, True),    # the skip; one 192-channel chunk; maps of two tiles
    (48, 192, 48, 1, 12, 20, True),    # a map that is no whole tile in either direction
    (64, 256, 64, 1, 8, 8, True),      # Cmid over two chunks; a map smaller than a tile
    (64, 256, 64, 1, 20, 12, True),
    (96, 384, 96, 1, 12, 12, True),    # two 192-channel chunks; the largest halo row; three project tiles
    (32, 128, 64, 2, 24, 24, False),   # the -L stride-2 blocks
    (64, 256, 96, 2, 24, 24, False),
    (48, 192, 80, 2, 16, 16, False),   # Cout no multiple of 32
    (40, 160, 40, 1, 8, 8, True),      # Cmid and Cin no multiples of 16 / 32: a partial chunk
    (8, 392, 8, 1, 8, 12, True),       # four 128-channel chunks, the last one of 8 channels
]


def _inputs(B, Cin, Cmid, Cout, H, W, seed, dtype, border=8.0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(B, Cin, H, W, device='cuda', generator=g)
    edge = torch.ones(H, W, device='cuda')   # large border pixels: a wrong halo or padding element shows
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = border
    x = (x * edge).to(dtype)
    w3 = (torch.randn(Cmid, Cin, 3, 3, device='cuda', generator=g) / (9 * Cin) ** 0.5).to(dtype)
    b3 = 0.5 * torch.randn(Cmid, device='cuda', generator=g)
    w1 = (torch.randn(Cout, Cmid, device='cuda', generator=g) / Cmid ** 0.5).to(dtype)
    b1 = 0.5 * torch.randn(Cout, device='cuda', generator=g)
    return x, w3, b3, w1, b1


def _chain(x, w3p, b3, act, stride, w1, b1, residual):
    from metrabs_amd import kernels
    mid = kernels.conv3x3_bias_act16(x, w3p, b3, act, stride)
    return kernels.conv1x1_bias_act16(mid, w1, b1, None, residual=residual)


def _ulp(v, dt):
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(torch.finfo(dt).tiny))) - _MANT[dt])


def _reference(x, w3, b3, act, stride, w1, b1, r):
    """(fp64 result, the module docstring's bound)."""
    dt = x.dtype
    K3, Cmid = 9 * x.shape[1], w1.shape[1]
    z3 = F.conv2d(x.double(), w3.double(), None, stride, 1) + b3.double()[None, :, None, None]
    s3 = F.conv2d(x.double().abs(), w3.double().abs(), None, stride, 1) + b3.double().abs()[None, :, None, None]
    m = _TORCH_ACT[act](z3)
    d_mid = _ulp(m, dt) + _LIPSCHITZ[act] * K3 * 2.0 ** -24 * s3 + 1e-6 * m.abs() + 2.0 ** -24
    w1d = w1.double()[:, :, None, None]
    ref = F.conv2d(m, w1d) + b1.double()[None, :, None, None]
    carried = F.conv2d(d_mid, w1d.abs())
    s1 = F.conv2d(m.abs() + d_mid, w1d.abs()) + b1.double().abs()[None, :, None, None]
    rabs = 0.0
    if r is not None:
        ref = ref + r.double()
        rabs = r.double().abs()
    return ref, carried + 1.1 * Cmid * 2.0 ** -24 * s1 + 2.0 ** -23 * (s1 + rabs) + 1e-6 * ref.abs() + 2.0 ** -24 \
        + _ulp(ref, dt)


def _check_fp64(x, w3, b3, act, stride, w1, b1, r, got, label):
    """The module docstring's bound, every element (tests/conv_fuzz.py uses the same two functions)."""
    dt = x.dtype
    ref, bound = _reference(x, w3, b3, act, stride, w1, b1, r)
    assert got.shape == ref.shape and got.dtype == dt
    err = (got.double() - ref).abs()
    print(f'k16h fp64 {label} {dt}: max err / bound = {float((err / bound).max()):.3f}')
    excess = float((err - bound).max())
    assert excess <= 0, excess


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_k16h_has_the_chains_bits_and_meets_the_fp64_bound(shape, B, dtype, hip_lib):
    from metrabs_amd import kernels
    Cin, Cmid, Cout, stride, H, W, skip = shape
    x, w3, b3, w1, b1 = _inputs(B, Cin, Cmid, Cout, H, W, 100 + Cin + H, dtype)
    w3p = kernels.pack_conv3x3_weight(w3)
    assert kernels.fused_mbconv16_supported(x, w3p, w1, stride), shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    assert (Ho * Wo) % 8 == 0 and kernels.conv1x1_16_supported(x.new_empty(B, Cmid, Ho, Wo), w1)
    r = x if skip else None
    got = kernels.fused_mbconv16(x, w3p, b3, 'silu', stride, w1, b1, residual=r)
    want = _chain(x, w3p, b3, 'silu', stride, w1, b1, r)
    diff = (got.float() - want.float()).abs()
    assert torch.equal(got, want), (shape, int((got != want).sum()), float(diff.max()))
    _check_fp64(x, w3, b3, 'silu', stride, w1, b1, r, got, f'{shape} B={B}')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('skip', [False, True])
@pytest.mark.parametrize('act', ACTS)
def test_k16h_every_epilogue(act, skip, dtype, hip_lib):
    from metrabs_amd import kernels
    x, w3, b3, w1, b1 = _inputs(3, 48, 192, 48, 16, 16, 11, dtype)
    w3p = kernels.pack_conv3x3_weight(w3)
    r = x if skip else None
    got = kernels.fused_mbconv16(x, w3p, b3, act, 1, w1, b1, residual=r)
    assert torch.equal(got, _chain(x, w3p, b3, act, 1, w1, b1, r))
    _check_fp64(x, w3, b3, act, 1, w1, b1, r, got, f'48-192-48 {act} skip={skip}')
    if skip:   # a residual that is not the input itself
        other = torch.randn_like(x)
        got = kernels.fused_mbconv16(x, w3p, b3, act, 1, w1, b1, residual=other)
        assert torch.equal(got, _chain(x, w3p, b3, act, 1, w1, b1, other))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('act', [None, 'relu'])
@pytest.mark.parametrize('stride', [1, 2])
def test_k16h_is_exact_on_small_integers(stride, act, dtype, hip_lib):
    """Small-integer data, asymmetric W3 (every tap and input channel distinct) and W1: every product, every partial
    sum, the intermediate and the output are integers of at most 2^8 in magnitude (exact in bf16, hence in f16, whose
    limit is 2^11), checked here on the CPU side of the reference -- so the result must EQUAL the integer
    evaluation: a swapped tap, a transposed fragment, a wrong chunk or halo cannot hide in rounding.  Cmid = 200 is
    two chunks, the second partial; Cout = 40 is a partial project tile."""
    from metrabs_amd import kernels
    Cin, Cmid, Cout, H, W = 24, 200, 40, 12, 24
    g = torch.Generator(device='cuda').manual_seed(3)
    x = torch.randint(-1, 2, (2, Cin, H, W), device='cuda', generator=g).float()
    w3 = torch.zeros(Cmid, Cin, 3, 3, device='cuda')
    c = torch.arange(Cmid, device='cuda')
    for t in range(9):   # channel c looks at tap t of input channel (c + 5 t) % Cin only, weight t + 1 or -(t + 1)
        w3[c, (c + 5 * t) % Cin, t // 3, t % 3] = torch.where(c % 2 == 0, t + 1.0, -(t + 1.0))
    b3 = c.float() % 7 - 3
    w1 = torch.zeros(Cout, Cmid, device='cuda')
    m = torch.arange(Cout, device='cuda')
    w1[m, (3 * m) % Cmid] = torch.where(m % 3 == 0, -1.0, 1.0)
    w1[m, (3 * m + 111) % Cmid] = torch.where(m % 2 == 0, 2.0, -2.0)   # (in the second chunk for most rows)
    b1 = m.float() % 5 - 2
    mid = _TORCH_ACT[act](F.conv2d(x.double(), w3.double(), b3.double(), stride, 1))
    ref = F.conv2d(mid, w1.double()[:, :, None, None], b1.double())
    limit = 2 ** 8   # bf16's exact integers; f16's 2^11 holds a fortiori
    assert float(mid.abs().max()) <= 45 + 3 and float(mid.abs().max()) <= limit
    assert float((mid.abs().amax(1) * 3 + 2).max()) <= limit and float(ref.abs().max()) <= limit
    assert float(ref.abs().max()) > 20   # (not a trivially small case)
    got = kernels.fused_mbconv16(x.to(dtype), kernels.pack_conv3x3_weight(w3.to(dtype)), b3, act, stride,
                                 w1.to(dtype), b1)
    assert torch.equal(got.double(), ref)


@pytest.mark.parametrize('dtype', DTYPES)
def test_k16h_is_deterministic_graph_safe_and_stays_inside_y(dtype, hip_lib):
    from metrabs_amd import kernels
    for (B, Cin, Cmid, Cout, stride, H, W, skip) in [(3, 48, 192, 48, 1, 12, 20, True),
                                                      (2, 64, 256, 96, 2, 24, 24, False)]:
        x, w3, b3, w1, b1 = _inputs(B, Cin, Cmid, Cout, H, W, 5, dtype)
        w3p = kernels.pack_conv3x3_weight(w3)
        r = x if skip else None
        a = kernels.fused_mbconv16(x, w3p, b3, 'silu', stride, w1, b1, residual=r)
        assert torch.equal(a, kernels.fused_mbconv16(x, w3p, b3, 'silu', stride, w1, b1, residual=r))
        # out= inside guard bands (64 elements either side: y's base stays 16-byte aligned)
        flat = torch.full((a.numel() + 128,), 7.0, device='cuda', dtype=dtype)
        out = flat[64:64 + a.numel()].view_as(a)
        assert kernels.fused_mbconv16(x, w3p, b3, 'silu', stride, w1, b1, residual=r, out=out) is out
        assert torch.equal(out, a)
        assert bool((flat[:64] == 7.0).all()) and bool((flat[-64:] == 7.0).all())
        with torch.inference_mode():
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                kernels.fused_mbconv16(x, w3p, b3, 'silu', stride, w1, b1, residual=r, out=out)
                st.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                    kernels.fused_mbconv16(x, w3p, b3, 'silu', stride, w1, b1, residual=r, out=out)
            torch.cuda.current_stream().wait_stream(st)
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, a)
            assert bool((flat[:64] == 7.0).all()) and bool((flat[-64:] == 7.0).all())
        # a shifted, 16-byte-aligned base of x is accepted, one 8 bytes off is refused
        xflat = torch.zeros(x.numel() + 8, device='cuda', dtype=dtype)
        x8 = xflat[8:].view_as(x).copy_(x)
        assert kernels.fused_mbconv16_supported(x8, w3p, w1, stride)
        assert torch.equal(kernels.fused_mbconv16(x8, w3p, b3, 'silu', stride, w1, b1,
                                                  residual=x8 if skip else None), a)
        x4 = xflat[4:4 + x.numel()].view_as(x)
        assert not kernels.fused_mbconv16_supported(x4, w3p, w1, stride)
        with pytest.raises(RuntimeError):
            kernels.fused_mbconv16(x4, w3p, b3, 'silu', stride, w1, b1)


def test_k16h_entry_point_argument_checks(hip_lib):
    """No GPU work: every call below is refused before a launch (the output stays untouched)."""
    from metrabs_amd import kernels
    null = ctypes.c_void_p(0)
    t = torch.zeros(1 << 16, device='cuda', dtype=torch.float16)
    sentinel = torch.full((4096,), 7.0, device='cuda', dtype=torch.float16)
    p = ctypes.c_void_p(t.data_ptr())
    q = ctypes.c_void_p(sentinel.data_ptr())
    f = hip_lib.mtr_fused_mbconv16

    def call(x=p, dtype=1, w3=p, b3=p, act=0, w1=p, b1=p, res=null, B=1, Cin=8, Cmid=32, Cout=8, H=8, W=8, stride=1,
             y=q):
        return f(x, dtype, w3, b3, act, w1, b1, res, B, Cin, Cmid, Cout, H, W, stride, y, null)

    for name in ('x', 'w3', 'b3', 'w1', 'b1', 'y'):
        assert call(**{name: null}) == -1, name            # MTR_E_NULL
    assert call(dtype=0) == -3 and call(dtype=3) == -3     # f32, an unknown code
    assert call(Cin=12) == -2 and call(Cin=3) == -2
    assert call(Cmid=36) == -2 and call(Cmid=0) == -2
    assert call(Cout=0) == -2 and call(Cout=136) == -2     # the project's accumulators: Cout <= 128
    assert call(stride=3) == -2 and call(stride=0) == -2
    assert call(W=7) == -2 and call(W=12, stride=2) == -2  # Wo = 6
    assert call(B=-1) == -2
    assert call(Cin=512, Cout=128, Cmid=2048, H=16, W=16) == -2   # the halo of 512 channels: not in LDS
    assert call(res=p, stride=2, H=16, W=16) == -2         # a skip with stride 2
    assert call(res=p, Cout=16) == -2                      # a skip with Cout != Cin
    assert call(act=7) == -4
    assert call(dtype=2, y=p) == -4                        # y aliases x
    assert call(dtype=2, res=q) == -4                      # y aliases the residual
    odd = ctypes.c_void_p(t.data_ptr() + 8)
    for name in ('x', 'w3', 'w1', 'y', 'res'):
        assert call(**{name: odd}) == -6, name             # MTR_E_ALIGN
    assert call(B=0) == 0                                  # nothing to do
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())

    x, w3, b3, w1, b1 = _inputs(2, 8, 32, 8, 8, 8, 1, torch.float16)
    w3p = kernels.pack_conv3x3_weight(w3)
    ok = kernels.fused_mbconv16(x, w3p, b3, None, 1, w1, b1, residual=x)
    assert torch.equal(ok, _chain(x, w3p, b3, None, 1, w1, b1, x))
    with pytest.raises(ValueError):
        kernels.fused_mbconv16(x, w3, b3, None, 1, w1, b1)                       # an OIHW weight
    with pytest.raises(ValueError):
        kernels.fused_mbconv16(x, w3p, b3, None, 1, w1[:, :16].contiguous(), b1)  # W1 of another Cmid
    with pytest.raises(ValueError):
        kernels.fused_mbconv16(x, w3p, b3, None, 3, w1, b1)
    with pytest.raises(ValueError):
        kernels.fused_mbconv16(x, w3p, b3, None, 2, w1, b1, residual=x[:, :, ::2, ::2].contiguous())
    with pytest.raises(ValueError):
        kernels.fused_mbconv16(x, w3p, b3, None, 1, w1[:4].contiguous(), b1[:4], residual=x[:, :4].contiguous())
    with pytest.raises(ValueError):
        kernels.fused_mbconv16(x, w3p, b3, None, 1, w1, b1, residual=x.bfloat16())
    with pytest.raises(ValueError):
        kernels.fused_mbconv16(x, w3p.bfloat16(), b3, None, 1, w1, b1)
    with pytest.raises(ValueError):
        kernels.fused_mbconv16(x, w3p, b3[:8], None, 1, w1, b1)
    with pytest.raises(RuntimeError):
        kernels.fused_mbconv16(x, w3p, b3, None, 1, w1, b1, residual=x, out=x)  # y aliases x
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        kernels.fused_mbconv16(x.cpu(), w3p.cpu(), b3.cpu(), None, 1, w1.cpu(), b1.cpu())
    assert not kernels.fused_mbconv16_supported(x, w3p, w1, 3)
    assert not kernels.fused_mbconv16_supported(x.to(memory_format=torch.channels_last), w3p, w1, 1)
    assert not kernels.fused_mbconv16_supported(x.float(), w3p, w1, 1)
    assert kernels.fused_mbconv16_supported(x, w3p, w1, 1)


def test_k16h_shape_query_agrees_with_supported(hip_lib):
    from metrabs_amd import kernels
    declined = 0
    # (Cin, Cmid, Cout, stride, H, W)
    for (Cin, Cmid, Cout, stride, H, W) in [(48, 192, 48, 1, 64, 64), (64, 256, 96, 2, 96, 96), (96, 384, 96, 1, 48, 48),
                                            (512, 2048, 128, 1, 16, 16), (128, 512, 128, 2, 64, 64),
                                            (48, 192, 160, 1, 16, 16), (24, 96, 48, 2, 12, 12), (24, 100, 48, 1, 8, 8)]:
        n = hip_lib.mtr_fused_mbconv16_lds_bytes(1, Cin, Cmid, Cout, H, W, stride)
        assert 0 <= n <= 160 * 1024
        x = torch.empty(1, Cin, H, W, device='cuda', dtype=torch.float16)
        w3p = torch.empty(Cmid, 3, 3, Cin, device='cuda', dtype=torch.float16)
        w1 = torch.empty(Cout, Cmid, device='cuda', dtype=torch.float16)
        assert kernels.fused_mbconv16_supported(x, w3p, w1, stride) == (n > 0), (Cin, Cmid, Cout, stride, H, W)
        declined += n == 0
    assert hip_lib.mtr_fused_mbconv16_lds_bytes(1, 512, 2048, 128, 16, 16, 1) == 0   # must be declined
    assert hip_lib.mtr_fused_mbconv16_lds_bytes(64, 48, 192, 48, 64, 64, 1) > 0
    assert declined >= 4


def _calibrated(name, res, batch_size=4):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    return backbones.calibrate_batchnorm(backbones.build_backbone(name).cuda(), res, 'cuda', batch_size=batch_size)


def _paths(net):
    return [(type(m).__name__, getattr(m, 'last_path', None)) for m in net.modules()]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['efficientnetv2-s', 'efficientnetv2-l'])
def test_armed_copy_takes_k16h_where_it_applies(name, dtype, hip_lib):
    from metrabs_amd import backbones, kernels
    FM = backbones.FusedMBConv
    res = 256
    net = _calibrated(name, res)
    f32 = backbones.fold_batchnorm(net, fused_epilogue=True)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype)
    plain2 = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, fuse_blocks=False)
    armed_net = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, fuse_blocks=True)
    # without the option: no armed block, nothing new on any module
    for c in (plain, plain2):
        assert not any('fused_pair' in m.__dict__ or m.fused_pair for m in c.modules() if isinstance(m, FM))
    assert list(plain.state_dict()) == list(armed_net.state_dict())
    assert [type(m) for m in plain.modules()] == [type(m) for m in armed_net.modules()]
    armed = [m for m in armed_net.modules() if isinstance(m, FM) and m.fused_pair]
    assert len(armed) == {'efficientnetv2-s': 8, 'efficientnetv2-l': 14}[name]
    for m in armed:
        assert m.fused_pair[0] is m.block[0][0] and m.fused_pair[1] is m.block[1][0]
    x = torch.rand(8, 3, res, res, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    seen = {}
    hs = [m.register_forward_pre_hook(lambda mod, args: seen.__setitem__(mod, args[0])) for m in armed]
    try:
        with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
            a = f32(x).float()
            off = plain(x)
            off2 = plain2(x)
            assert _paths(plain) == _paths(plain2) and torch.equal(off, off2)
            assert all(m.last_path is None for m in plain.modules() if isinstance(m, FM))
            on = armed_net(x)
            took = 0
            for m in armed:
                xin = seen[m]
                e, p = m.fused_pair
                key = (e.conv.in_channels, e.conv.out_channels, p.conv.out_channels, e.stride, xin.shape[2], xin.shape[3])
                want = kernels.fused_mbconv16_supported(xin.to(dtype).contiguous(), e.weight_packed, p.conv.weight,
                                                        e.stride) and key not in FM.k16h_slower
                assert m.last_path == ('k16h' if want else 'chain'), (key, m.last_path)
                took += want
            assert took >= 1 or all(
                (m.fused_pair[0].conv.in_channels, m.fused_pair[0].conv.out_channels, m.fused_pair[1].conv.out_channels,
                 m.fused_pair[0].stride, seen[m].shape[2], seen[m].shape[3]) in FM.k16h_slower for m in armed)
            armed_net(x.to(memory_format=torch.channels_last))
            assert all(m.last_path == 'chain' for m in armed)
            FM.use_k16h = False
            chain = armed_net(x)
            assert all(m.last_path == 'chain' for m in armed)
            FM.use_k16h = True
            # the armed copy on the chain is the default copy: same paths below the blocks, same bits
            assert torch.equal(chain, off)
            assert [p for p in _paths(armed_net) if p[0] != 'FusedMBConv'] == \
                [p for p in _paths(plain) if p[0] != 'FusedMBConv']
    finally:
        FM.use_k16h = True
        for h in hs:
            h.remove()
    assert on.dtype == dtype and torch.isfinite(on).all()
    # no further from the f32 network than the unfused 16-bit copy (test_copy_takes_k14h_where_it_applies's criterion)
    mean_on, mean_off = float((on.float() - a).abs().mean()), float((off.float() - a).abs().mean())
    print(f'{name} {dtype}: mean |copy - f32| k16h on {mean_on:.6g} off {mean_off:.6g} max|f32| {float(a.abs().max()):.4g}')
    assert mean_on <= 1.1 * mean_off + 1e-6 * float(a.abs().max()), (mean_on, mean_off)


@pytest.mark.parametrize('name', ['resnet18', 'mobilenetv3'])
def test_other_backbones_fold_with_the_option_and_arm_nothing(name, hip_lib):
    from metrabs_amd import backbones
    net = _calibrated(name, 128)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=torch.float16)
    opt = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=torch.float16, fuse_blocks=True)
    assert not any(getattr(m, 'fused_pair', ()) for m in opt.modules())
    assert list(plain.state_dict()) == list(opt.state_dict())
    x = torch.rand(2, 3, 128, 128, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        assert torch.equal(plain(x), opt(x))
    assert _paths(plain) == _paths(opt)


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


def test_k16h_through_the_loader_and_the_api(tmp_path, hip_lib):
    from metrabs_amd import backbones, loading
    d = _model_dir(tmp_path)
    with pytest.raises(ValueError):
        loading.load_crop_model(d, fuse_blocks=True)
    est = loading.load_multiperson_model(d, dtype=torch.float16, fuse_blocks=True)
    est.crop_model.deterministic_backbone = True
    est.graph_batches = True
    eager = loading.load_multiperson_model(d, dtype=torch.float16, fuse_blocks=True)
    eager.crop_model.deterministic_backbone = True
    eager.graph_batches = False
    for seed in (5, 9):
        images = torch.stack([cases.synth_images(1, 240, 320, seed + i)[0] for i in range(2)]).cuda()
        boxes = [torch.tensor([[60.0, 20.0, 120.0, 200.0], [150.0, 30.0, 100.0, 180.0]]),
                 torch.tensor([[40.0, 10.0, 140.0, 210.0]])]
        a, b = _poses(eager, images, boxes), _poses(est, images, boxes)
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), float((a - b).abs().max())   # a graphed call returns the eager call's bits
    for model in (est, eager):
        paths = [m.last_path for m in model.crop_model.backbone.modules()
                 if isinstance(m, backbones.FusedMBConv) and m.fused_pair]
        assert 'k16h' in paths, paths
    assert est.graphs.stats['captures'] >= 1 and est.graphs.stats['replays'] >= 1, est.graphs.stats

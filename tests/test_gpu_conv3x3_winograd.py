"""GPU: K19 (csrc/conv3x3_winograd.hip), the dense 3x3 stride-1 convolution of the f32 inference copy as Winograd
F(2x2, 3x3) on the f32 MFMA with the K10 epilogue, through the C-ABI wrapper (kernels.conv3x3_winograd_bias_act).

The fp64 bound (_check), every element:

    |got - ref| <= 1.1 (Cin + 10) 2^-24 S + 1e-6 |ref| + 2^-24

ref is F.conv2d of the f32 operands in fp64, through bias, activation and skip.  S is the same Winograd evaluation in
fp64 with |x|, |g| and the absolute values of the three transform matrices, plus |bias|: it bounds the magnitude of every
intermediate of the chain that leads to an output.  Derivation: each path through the evaluation is rounded once for U
(fp64 -> f32), twice in the input transform (two passes, one addition each), once for the product, Cin times in the
accumulation chain, four times in the output transform (two passes of two additions) and once for "+ bias": at most
Cin + 9 roundings of relative size 2^-24 on quantities whose absolute sum is S, rounded up to Cin + 10; the activation's
Lipschitz constant is at most 1.1 (silu 1.0998); 1e-6 |ref| covers the activation's own evaluation (exp and a
reciprocal of 1 ulp) and the rounding of the skip's addition; 2^-24 is absolute slack below the smallest bias scale.
An f32 restatement on the CPU stays at <= 0.021 of this bound; a wrong tap is orders of magnitude outside it.

Also: exact integers (every step of F(2x2, 3x3) is exact there), the RMS error against an f32 restatement of the same
arithmetic, determinism (calls, a sliced batch, a graph replay), a NaN guard band, argument checks, the
WinogradConv3x3BiasAct module inside the copies (paths, switches, refusals), whole-backbone accuracy against an fp64
forward, and the loader and the API."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cases

pytestmark = pytest.mark.gpu

ACTS = [None, 'relu', 'silu', 'hardswish']
_TORCH_ACT = {None: lambda t: t, 'relu': F.relu, 'silu': F.silu, 'hardswish': F.hardswish}
_BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
_G = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
_AT = [[1, 1, 1, 0], [0, 1, -1, -1]]


def _tiles(x):
    """[B, C, H, W] -> the 4x4 input patches of the 2x2 output tiles, [B, C, H/2, W/2, 4, 4] (zero padding 1)."""
    return F.pad(x, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)


def _winograd64(x, w, absolute=False):
    """The F(2x2, 3x3) evaluation in fp64; absolute=True: with |x|, |g| and the absolute transform matrices."""
    mat = lambda m: torch.tensor(m, dtype=torch.float64, device=x.device)
    BT, G, AT = mat(_BT), mat(_G), mat(_AT)
    x, w = x.double(), w.double()
    if absolute:
        BT, G, AT, x, w = BT.abs(), G.abs(), AT.abs(), x.abs(), w.abs()
    V = torch.einsum('ik,bcyxkl,jl->ijbcyx', BT, _tiles(x), BT)
    U = torch.einsum('ik,mckl,jl->ijmc', G, w, G)
    B, C, TY, TX = V.shape[2:]
    Mm = torch.bmm(U.reshape(16, -1, C), V.reshape(16, B, C, TY * TX).permute(0, 2, 1, 3).reshape(16, C, -1))
    Mm = Mm.view(4, 4, -1, B, TY, TX)
    Y = torch.einsum('pi,ijmbyx,qj->bmypxq', AT, Mm, AT)
    return Y.reshape(B, -1, 2 * TY, 2 * TX)


def _restatement32(x, w):
    """The kernel's arithmetic in torch f32: the fp64 weight transform rounded once, two-pass transforms (every row of
    B^T has two non-zeros: one addition per pass and element), a sequential ci chain, a two-pass output transform."""
    from metrabs_amd import kernels
    U = kernels.pack_conv3x3_winograd_weight(w).view(4, 4, w.shape[0], w.shape[1])
    BT = torch.tensor(_BT, dtype=torch.float32, device=x.device)
    t = torch.einsum('ik,bcyxkl->bcyxil', BT, _tiles(x))
    V = torch.einsum('bcyxil,jl->ijbcyx', t, BT)
    acc = torch.zeros(4, 4, x.shape[0], w.shape[0], V.shape[4], V.shape[5], device=x.device)
    for ci in range(x.shape[1]):
        acc = acc + U[:, :, None, :, ci, None, None] * V[:, :, :, None, ci]
    s0 = (acc[:, 0] + acc[:, 1]) + acc[:, 2]          # M A: [4, b, m, y, x] per output column
    s1 = (acc[:, 1] - acc[:, 2]) - acc[:, 3]
    rows = []
    for s in (s0, s1):
        rows.append(torch.stack([(s[0] + s[1]) + s[2], (s[1] - s[2]) - s[3]]))   # [p, b, m, y, x]
    Y = torch.stack(rows, dim=-1)                      # [p, b, m, y, x, q]
    return Y.permute(1, 2, 3, 0, 4, 5).reshape(x.shape[0], w.shape[0], x.shape[2], x.shape[3])


def _inputs(B, K, M, H, W, seed, residual, border=1.0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(B, K, H, W, device='cuda', generator=g)
    if border != 1.0:   # large border pixels: a wrong halo (a missed or a doubled edge tap) shows
        edge = torch.ones(H, W, device='cuda')
        edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = border
        x = x * edge
    w = torch.randn(M, K, 3, 3, device='cuda', generator=g) / (9 * K) ** 0.5
    b = 0.5 * torch.randn(M, device='cuda', generator=g)
    r = torch.randn(B, M, H, W, device='cuda', generator=g) if residual else None
    return x, w, b, r


def _ref64(x, w, b, act, r):
    ref = _TORCH_ACT[act](F.conv2d(x.double(), w.double(), b.double(), 1, 1))
    return ref if r is None else ref + r.double()


def _reference(x, w, b, act, r):
    """(fp64 result, the bound of the module docstring)."""
    K = x.shape[1]
    ref = _ref64(x, w, b, act, r)
    S = _winograd64(x, w, absolute=True) + b.double().abs()[None, :, None, None]
    return ref, 1.1 * (K + 10) * 2.0 ** -24 * S + 1e-6 * ref.abs() + 2.0 ** -24


def _check(x, w, b, act, r, got):
    """The bound of the module docstring, on every element (tests/conv_fuzz.py uses the same two functions)."""
    ref, bound = _reference(x, w, b, act, r)
    assert got.shape == ref.shape and got.dtype == torch.float32
    err = (got.double() - ref).abs()
    print(f'k19 check {tuple(x.shape)} -> {tuple(got.shape)} {act} skip {r is not None}: '
          f'max err / bound = {float((err / bound).max()):.4f}')
    excess = float((err - bound).max())
    assert excess <= 0, excess


def _run(x, w, b, act, r, **kw):
    from metrabs_amd import kernels
    wu = kernels.pack_conv3x3_winograd_weight(w)
    assert kernels.conv3x3_winograd_supported(x, wu), tuple(x.shape)
    return kernels.conv3x3_winograd_bias_act(x, wu, b, act, residual=r, **kw)


def test_fp64_winograd_helper_is_the_convolution():
    """The test's own fp64 Winograd evaluation (the one S is made with) equals F.conv2d to fp64 rounding."""
    x, w, _, _ = _inputs(2, 8, 12, 12, 20, 1, False)
    ref = F.conv2d(x.double(), w.double(), None, 1, 1)
    assert float((_winograd64(x, w) - ref).abs().max()) < 1e-12
    assert float((_restatement32(x, w).double() - ref).abs().max()) < 1e-4


@functools.lru_cache(maxsize=None)
def _armed_shapes(name, res):
    """(Cin, Cout, H, W, act, residual) of every armed layer's input at `res` px, from a hooked forward."""
    from metrabs_amd import backbones
    W3 = backbones.WinogradConv3x3BiasAct
    net = backbones.fold_batchnorm(backbones.build_backbone(name).eval(), fused_epilogue=True, winograd3x3=True).cuda()
    shapes = set()

    def hook(mod, args, kwargs):
        x = args[0]
        shapes.add((x.shape[1], mod.conv.out_channels, x.shape[2], x.shape[3], mod.act_name,
                    kwargs.get('residual') is not None))

    hs = [m.register_forward_pre_hook(hook, with_kwargs=True) for m in net.modules() if isinstance(m, W3)]
    assert hs
    W3.use_k19 = False
    try:
        with torch.inference_mode():
            net(torch.rand(1, 3, res, res, device='cuda'))
    finally:
        W3.use_k19 = True
    for h in hs:
        h.remove()
    return tuple(sorted(shapes, key=str))


_BENCH_BATCH = {'efficientnetv2-s': 64, 'efficientnetv2-l': 32, 'resnet18': 64}


@pytest.mark.parametrize('name,res', [('efficientnetv2-s', 256), ('efficientnetv2-s', 224), ('efficientnetv2-s', 160),
                                      ('efficientnetv2-l', 384), ('resnet18', 256)])
@pytest.mark.parametrize('B', [1, 3, 'bench'])
def test_k19_matches_fp64_on_every_armed_shape(name, res, B, hip_lib):
    shapes = _armed_shapes(name, res)
    assert len(shapes) >= 3
    ran = 0
    for i, (K, M, H, W, act, res_) in enumerate(shapes):
        n = _BENCH_BATCH[name] if B == 'bench' else B
        if B == 'bench' and n * M * H * W > 2 ** 26:
            continue   # (the fp64 reference of the largest maps at the bench batch: covered at B = 1, 3)
        x, w, b, r = _inputs(n, K, M, H, W, 2000 + i, res_)
        _check(x, w, b, act, r, _run(x, w, b, act, r))
        ran += 1
    assert ran >= 2


# (Cin, Cout, H, W): a map smaller than a workgroup's 64 tiles with one k step; partial workgroups and Cout not a
# multiple of 16; Cin not a multiple of the 8-channel chunk's 16 / 8; non-square maps; the longest chain
EDGE_SHAPES = [(4, 8, 4, 4), (8, 24, 20, 20), (24, 72, 28, 28), (40, 24, 12, 12), (24, 96, 12, 20), (40, 160, 20, 12),
               (96, 72, 8, 8), (512, 64, 8, 8)]


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('residual', [False, True])
@pytest.mark.parametrize('shape', EDGE_SHAPES)
def test_k19_every_epilogue_and_edge_geometry(act, residual, shape, hip_lib):
    K, M, H, W = shape
    x, w, b, r = _inputs(3, K, M, H, W, 7, residual, border=8.0)
    _check(x, w, b, act, r, _run(x, w, b, act, r))


def test_k19_takes_x_itself_as_the_residual(hip_lib):
    x, w, b, _ = _inputs(3, 24, 24, 20, 12, 11, False, border=8.0)
    got = _run(x, w, b, 'silu', x)
    _check(x, w, b, 'silu', x, got)
    assert torch.equal(got, _run(x, w, b, 'silu', x.clone()))
    x12, w12, b12, _ = _inputs(2, 12, 12, 6, 8, 12, False)   # Cin % 8 == 4: half a chunk of zeros
    _check(x12, w12, b12, 'relu', x12, _run(x12, w12, b12, 'relu', x12))


@pytest.mark.parametrize('skip', [False, True])
@pytest.mark.parametrize('shape', [(4, 8, 4, 4), (24, 24, 16, 16), (48, 192, 12, 20), (512, 64, 8, 8)])
def test_k19_is_exact_on_small_integers(shape, skip, hip_lib):
    """x in [-4, 4], w = 4 x integers in [-2, 2], integer bias and skip: U, the transformed input (|.| <= 16), every
    product and every partial sum (<= 512 * 16 * 18 * 4 < 2^24) are integers, so every step of F(2x2, 3x3) is exact and
    the result must equal the fp64 convolution -- a swapped tap, a transposed fragment or a wrong halo cannot hide in
    rounding.  The weights have no symmetry in ky, kx, ci or m."""
    K, M, H, W = shape
    g = torch.Generator(device='cuda').manual_seed(3)
    x = torch.randint(-4, 5, (2, K, H, W), device='cuda', generator=g).float()
    w = 4.0 * torch.randint(-2, 3, (M, K, 3, 3), device='cuda', generator=g).float()
    b = (torch.arange(M, device='cuda') % 7 - 3).float()
    r = torch.randint(-9, 10, (2, M, H, W), device='cuda', generator=g).float() if skip else None
    ref = _ref64(x, w, b, None, r)
    assert float(ref.abs().max()) < 2 ** 24
    assert torch.equal(_run(x, w, b, None, r), ref.float())


@pytest.mark.parametrize('shape', [(24, 24, 16, 16), (64, 256, 8, 8), (512, 64, 8, 8)])
def test_k19_arithmetic_is_as_accurate_as_its_f32_restatement(shape, hip_lib):
    """The accuracy of the arithmetic, not only of the taps: the RMS error against fp64 is at most 1.5 x that of the
    torch f32 restatement of the same evaluation (_restatement32: the same arithmetic up to the order inside the
    transforms and fma contraction, hence the 1.5)."""
    K, M, H, W = shape
    x, w, b, _ = _inputs(3, K, M, H, W, 21, False)
    ref = F.conv2d(x.double(), w.double(), None, 1, 1)
    got = _run(x, w, torch.zeros_like(b), None, None)
    rms = lambda t: float((t.double() - ref).pow(2).mean().sqrt())
    e_k19, e_f32 = rms(got), rms(_restatement32(x, w))
    print(f'k19 rms {shape}: kernel {e_k19:.4g} restatement {e_f32:.4g} ratio {e_k19 / e_f32:.3f}')
    assert e_k19 <= 1.5 * e_f32, (e_k19, e_f32)


def test_k19_is_deterministic_and_graph_safe(hip_lib):
    from metrabs_amd import kernels
    for (B, K, M, H, W, res_) in [(3, 24, 24, 32, 32, True), (3, 48, 192, 16, 16, False), (3, 40, 72, 20, 12, True)]:
        x, w, b, r = _inputs(B, K, M, H, W, 3, res_)
        wu = kernels.pack_conv3x3_winograd_weight(w)
        a = kernels.conv3x3_winograd_bias_act(x, wu, b, 'silu', residual=r)
        assert torch.equal(a, kernels.conv3x3_winograd_bias_act(x, wu, b, 'silu', residual=r))
        # images 1 .. 2 of 3 as a batch of their own: other tile numbers, other workgroups, the same bits
        part = kernels.conv3x3_winograd_bias_act(x[1:], wu, b, 'silu', residual=None if r is None else r[1:])
        assert torch.equal(part, a[1:])
        with torch.inference_mode():
            out = torch.empty_like(a)
            assert kernels.conv3x3_winograd_bias_act(x, wu, b, 'silu', residual=r, out=out) is out
            assert torch.equal(out, a)
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                kernels.conv3x3_winograd_bias_act(x, wu, b, 'silu', residual=r, out=out)
                st.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                    kernels.conv3x3_winograd_bias_act(x, wu, b, 'silu', residual=r, out=out)
            torch.cuda.current_stream().wait_stream(st)
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, a)


@pytest.mark.parametrize('shape', [(4, 8, 4, 4), (24, 40, 20, 12), (40, 24, 12, 12)])
def test_k19_writes_nothing_outside_y_and_reads_nothing_outside_its_inputs(shape, hip_lib):
    """x, y and the skip are carved out of one larger buffer filled with NaN: nothing outside y changes, and no NaN
    gets into y (a read outside x or the skip would bring one in)."""
    from metrabs_amd import kernels
    K, M, H, W = shape
    B = 3
    x0, w, b, r0 = _inputs(B, K, M, H, W, 5, True)
    nx, ny, gap = x0.numel(), r0.numel(), 1024
    buf = torch.full((4 * gap + nx + 2 * ny,), float('nan'), device='cuda')
    ox, orr, oy = gap, 2 * gap + nx, 3 * gap + nx + ny
    x, r, y = buf[ox:ox + nx].view_as(x0), buf[orr:orr + ny].view_as(r0), buf[oy:oy + ny].view_as(r0)
    x.copy_(x0), r.copy_(r0)
    before = buf.view(torch.int32).clone()
    wu = kernels.pack_conv3x3_winograd_weight(w)
    assert kernels.conv3x3_winograd_bias_act(x, wu, b, 'relu', residual=r, out=y) is y
    torch.cuda.synchronize()
    after = buf.view(torch.int32)
    assert torch.equal(after[:oy], before[:oy]) and torch.equal(after[oy + ny:], before[oy + ny:])
    assert not torch.isnan(y).any()
    assert torch.equal(y, kernels.conv3x3_winograd_bias_act(x0, wu, b, 'relu', residual=r0))


def test_k19_wrapper_argument_checks(hip_lib):
    from metrabs_amd import kernels
    x, w, b, r = _inputs(2, 8, 16, 8, 8, 1, True)
    wu = kernels.pack_conv3x3_winograd_weight(w)
    ok = kernels.conv3x3_winograd_bias_act(x, wu, b, None, residual=r)
    with pytest.raises(ValueError):
        kernels.conv3x3_winograd_bias_act(x.half(), wu, b, None)                        # dtype
    with pytest.raises(ValueError):
        kernels.conv3x3_winograd_bias_act(x, wu.half(), b, None)
    with pytest.raises(ValueError):
        kernels.conv3x3_winograd_bias_act(x.to(memory_format=torch.channels_last), wu, b, None)   # layout
    with pytest.raises(ValueError):
        kernels.conv3x3_winograd_bias_act(x, w, b, None)                                # the OIHW weight
    with pytest.raises(ValueError):
        kernels.conv3x3_winograd_bias_act(x, wu[:, :, :4].contiguous(), b, None)        # another Cin
    with pytest.raises(ValueError):
        kernels.conv3x3_winograd_bias_act(x, wu[:8].contiguous(), b, None)
    with pytest.raises(ValueError):
        kernels.conv3x3_winograd_bias_act(x, wu, b[:4], None)
    with pytest.raises(ValueError):
        kernels.conv3x3_winograd_bias_act(x, wu, b, None, residual=r[:, :, :4].contiguous())
    with pytest.raises(ValueError):
        kernels.conv3x3_winograd_bias_act(x, wu, b, None, residual=r.half())
    with pytest.raises(ValueError):
        kernels.conv3x3_winograd_bias_act(x, wu, b, None, out=torch.empty(2, 16, 8, 4, device='cuda'))
    with pytest.raises(ValueError):
        kernels.conv3x3_winograd_bias_act(x, wu, b, None, residual=r, out=r)            # an aliasing out
    x16, w16, b16, _ = _inputs(2, 16, 16, 8, 8, 2, False)
    with pytest.raises(ValueError):
        kernels.conv3x3_winograd_bias_act(x16, kernels.pack_conv3x3_winograd_weight(w16), b16, None, out=x16)
    with pytest.raises(RuntimeError):                                                   # no CPU fallback
        kernels.conv3x3_winograd_bias_act(x.cpu(), wu.cpu(), b.cpu(), None)
    with pytest.raises(RuntimeError):                                                   # MTR_E_SHAPE through check()
        kernels.conv3x3_winograd_bias_act(x[:, :, :7].contiguous(), wu, b, None)
    assert kernels.conv3x3_winograd_supported(x, wu)
    assert not kernels.conv3x3_winograd_supported(x[:, :, :7].contiguous(), wu)         # odd H
    assert not kernels.conv3x3_winograd_supported(x[:, :, :, :6].contiguous(), wu)      # W % 4 != 0
    assert not kernels.conv3x3_winograd_supported(x.to(memory_format=torch.channels_last), wu)
    assert not kernels.conv3x3_winograd_supported(x.half(), wu.half())
    assert not kernels.conv3x3_winograd_supported(x.half(), wu)
    assert not kernels.conv3x3_winograd_supported(x, w)
    flat = torch.zeros(x.numel() + 2, device='cuda')
    assert not kernels.conv3x3_winograd_supported(flat[2:].view_as(x), wu)              # 8 bytes past a boundary
    assert torch.equal(ok, kernels.conv3x3_winograd_bias_act(x, wu, b, None, residual=r))


def _calibrated(name, res, batch_size=4):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    return backbones.calibrate_batchnorm(backbones.build_backbone(name).cuda(), res, 'cuda', batch_size=batch_size)


def _pinned():
    return torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True)


def _all_paths(net):
    return [getattr(m, 'last_path', None) for m in net.modules()]


def test_armed_efficientnet_takes_k19_where_it_applies(hip_lib):
    from metrabs_amd import backbones
    W3, FB = backbones.WinogradConv3x3BiasAct, backbones.FusedMBConv
    net = _calibrated('efficientnetv2-s', 128)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, winograd3x3=True)
    feats = armed[1]
    x = torch.rand(2, 3, 128, 128, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    with torch.inference_mode(), _pinned():
        ref = plain(x).clone()
        assert 'k19' not in _all_paths(plain)            # the default copy: no K19 anywhere
        on = armed(x).clone()
        for blk in feats[1]:                              # stage 1 (expand 1): the layer itself, with the skip
            assert isinstance(blk.block[0][0], W3) and blk.block[0][0].last_path == 'k19'
        for stage in (feats[2], feats[3]):                # stages 2 - 3: stride-2 first block, then stride-1 blocks
            assert stage[0].last_path == 'k13_pre' and type(stage[0].pre_pair[0]) is backbones.ConvBiasAct
            for blk in list(stage)[1:]:
                assert isinstance(blk, FB) and blk.last_path == 'k19', blk.last_path
                assert blk.pre_pair[0].last_path == 'k19' and blk.pre_pair[1].last_path == 'k13'
        assert torch.isfinite(on).all() and not torch.equal(on, ref)
        rel = float((on - ref).norm() / ref.norm())
        print(f'armed vs default copy, EfficientNetV2-S 128 px: relative difference {rel:.3g}')
        assert rel < 1e-4
        # the switch, and a listed shape: exactly what the default copy runs, the same bits
        mods = [m for m in armed.modules() if isinstance(m, W3)]
        shipped = W3.k19_slower
        try:
            W3.use_k19 = False
            off = armed(x).clone()
            assert all(m.last_path == 'library' for m in mods) and 'k19' not in _all_paths(armed)
            assert torch.equal(off, ref)
            W3.use_k19 = True
            W3.k19_slower = frozenset({(24, 24, 64, 64), (48, 192, 32, 32), (64, 256, 16, 16)})
            listed = armed(x).clone()
            assert 'k19' not in _all_paths(armed)
            assert torch.equal(listed, ref)
            W3.k19_slower = frozenset({(48, 192, 32, 32)})
            armed(x)
            assert feats[2][1].last_path == 'k13_pre' and feats[3][1].last_path == 'k19'
        finally:
            W3.use_k19, W3.k19_slower = True, shipped
        # autocast and channels_last input: the library path
        with torch.autocast('cuda', dtype=torch.float16):
            armed(x)
        assert all(m.last_path == 'library' for m in mods)
        armed(x)
        assert all(m.last_path == 'k19' for m in mods)
        m0 = mods[0]
        xin = torch.rand(2, 24, 64, 64, device='cuda')
        assert m0.k19_takes(xin) and not m0.k19_takes(xin.to(memory_format=torch.channels_last))
        m0(xin.to(memory_format=torch.channels_last))
        assert m0.last_path == 'library'
        m0(xin)
        assert m0.last_path == 'k19'
    xg = torch.rand(2, 24, 64, 64, device='cuda', requires_grad=True)   # a gradient wanted: the library path
    assert not mods[0].k19_takes(xg)


def test_armed_resnet18_takes_k19_on_all_13_layers(hip_lib):
    from metrabs_amd import backbones
    W3 = backbones.WinogradConv3x3BiasAct
    net = _calibrated('resnet18', 128)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, winograd3x3=True)
    mods = [m for m in armed.modules() if isinstance(m, W3)]
    assert len(mods) == 13
    x = torch.rand(2, 3, 128, 128, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    with torch.inference_mode(), _pinned():
        y = armed(x)
    assert torch.isfinite(y).all()
    assert [m.last_path for m in mods] == ['k19'] * 13


@pytest.mark.parametrize('name', ['efficientnetv2-s', 'resnet18'])
def test_whole_backbone_accuracy_against_fp64(name, hip_lib):
    """The armed copy's features against an fp64 CPU forward of the same folded network: a relative RMS error of at
    most 2 x the default copy's (the parent's path) against that same forward -- both are rounding noise from
    different summation orders, hence the margin."""
    import copy
    from metrabs_amd import backbones
    net = _calibrated(name, 128)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, winograd3x3=True)
    x = torch.rand(2, 3, 128, 128, device='cuda', generator=torch.Generator(device='cuda').manual_seed(4))
    ref = copy.deepcopy(plain).cpu().double()
    with torch.inference_mode():
        want = ref(x.cpu().double())
        with _pinned():
            got_plain, got_armed = plain(x).double().cpu(), armed(x).double().cpu()
    assert 'k19' in _all_paths(armed) and 'k19' not in _all_paths(plain)
    rel = lambda t: float((t - want).norm() / want.norm())
    e_plain, e_armed = rel(got_plain), rel(got_armed)
    print(f'{name} 128 px B = 2, relative RMS error against fp64: default copy {e_plain:.4g}, armed copy {e_armed:.4g}')
    assert e_armed <= 2 * e_plain, (e_armed, e_plain)


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


def _api_inputs(seed=5):
    images = torch.stack([cases.synth_images(1, 240, 320, seed + i)[0] for i in range(2)]).cuda()
    boxes = [torch.tensor([[60.0, 20.0, 120.0, 200.0], [150.0, 30.0, 100.0, 180.0]]),
             torch.tensor([[40.0, 10.0, 140.0, 210.0]])]
    return images, boxes


def _poses(est, images, boxes, num_aug=2):
    with torch.inference_mode():
        r = est.estimate_poses_batched(images, boxes, num_aug=num_aug)
    return torch.cat(r['poses3d']).clone()


class _Fp64Backbone(torch.nn.Module):
    """A folded backbone evaluated in fp64 on the CPU, handing f32 features back: the truth of the API test."""

    def __init__(self, folded):
        super().__init__()
        import copy
        # (in a tuple: not a registered submodule, so the estimator still finds its crop model's parameters on the GPU)
        self._net = (copy.deepcopy(folded).cpu().double(),)

    def forward(self, x):
        return self._net[0](x.detach().double().cpu()).float().to(x.device)


def test_k19_through_the_loader_and_the_api(tmp_path, hip_lib):
    """Eager and graphed calls of the armed model return the same bits.
    Between copies, in the manner of tests/test_gpu_backbone16.py (MPJPE of each copy to a reference of the same
    model through estimate_poses_batched), with a reference whose own error is negligible: the same folded network with
    its backbone evaluated in fp64 (one rounding of the features to f32; sampler and head are the same kernels for every
    arm).  That test's f32 reference cannot serve here: it runs the default copy's own library kernel and summation
    order in the 3x3 layers, so it is closer to that copy than to the truth (measured: 0.0020 against 0.0012 mm).
    Asserted: MPJPE(armed, fp64) <= 2 x MPJPE(default copy, fp64) -- both are f32 rounding noise from different
    summation orders, the margin of test_whole_backbone_accuracy_against_fp64 -- and, what follows from it by the
    triangle inequality, MPJPE(armed, default copy) <= 3 x MPJPE(default copy, fp64).  A wrong armed layer moves the
    features by far more than the 1e-5 relative that this noise is."""
    from metrabs_amd import backbones, loading
    d = _model_dir(tmp_path)
    plain = loading.load_multiperson_model(d, fold_batchnorm=True, fused_epilogue=True)
    truth = loading.load_multiperson_model(d, fold_batchnorm=True, fused_epilogue=True)
    truth.crop_model.backbone = _Fp64Backbone(truth.crop_model.backbone)
    est = loading.load_multiperson_model(d, winograd3x3=True)
    eager = loading.load_multiperson_model(d, winograd3x3=True)
    for m in (plain, est, eager):
        m.crop_model.deterministic_backbone = True
    est.graph_batches, eager.graph_batches, truth.graph_batches = True, False, False
    for seed in (5, 9):
        images, boxes = _api_inputs(seed)
        a, b = _poses(eager, images, boxes), _poses(est, images, boxes)
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), float((a - b).abs().max())   # a graphed call returns the eager call's bits
    for model in (est, eager):
        paths = [m.last_path for m in model.crop_model.backbone.modules()
                 if isinstance(m, backbones.WinogradConv3x3BiasAct)]
        assert paths == ['k19'] * 8, paths
    assert est.graphs.stats['captures'] >= 1 and est.graphs.stats['replays'] >= 1, est.graphs.stats
    images, boxes = _api_inputs(5)
    # (one crop per box: the fp64 backbone runs on the CPU)
    p_true, p_plain, p_armed = (_poses(e, images, boxes, num_aug=1) for e in (truth, plain, eager))
    assert 'k19' not in _all_paths(plain.crop_model.backbone)
    assert p_true.shape == p_armed.shape and torch.isfinite(p_true).all()
    mpjpe = lambda p, q: float((p - q).norm(dim=-1).mean())
    e_armed, e_plain, apart = mpjpe(p_armed, p_true), mpjpe(p_plain, p_true), mpjpe(p_armed, p_plain)
    print(f'MPJPE to the fp64-backbone poses: armed copy {e_armed:.5g} mm, default copy {e_plain:.5g} mm; '
          f'armed to default copy {apart:.5g} mm; mean |p| {float(p_true.norm(dim=-1).mean()):.4g} mm')
    assert 0 < e_armed <= 2 * e_plain, (e_armed, e_plain)
    assert 0 < apart <= 3 * e_plain, (apart, e_plain)

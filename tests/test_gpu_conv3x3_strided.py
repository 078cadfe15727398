"""GPU: K22 (csrc/conv3x3_strided.hip), the dense 3x3 stride-2 convolution of the f32 inference copy as an implicit GEMM
on the f32 MFMA with the K10 epilogue, through the C-ABI wrapper (kernels.conv3x3_strided_bias_act).

The fp64 bound (_check), every element:

    |got - ref| <= 1.1 (9 Cin + 2) 2^-24 S + 1e-6 |ref| + 2^-24

ref is F.conv2d(x.double(), w.double(), b.double(), 2, 1) through activation and skip.  S = F.conv2d(|x|, |w|, stride 2,
padding 1) in fp64 + |bias|: it bounds the magnitude of every partial sum of the chain that leads to an output.
Derivation: the chain rounds 9 Cin times (one per fma: the product is exact inside it) and "+ bias" once, 9 Cin + 1
roundings of relative size 2^-24 on quantities of absolute sum at most S, rounded up by one; the activation's Lipschitz
constant is at most 1.1 (silu 1.0998); 1e-6 |ref| covers the activation's own evaluation (exp and a reciprocal of 1 ulp)
and the rounding of the skip's addition; 2^-24 is absolute slack below the smallest bias scale.  A worst-case bound: any
correct f32 evaluation sits inside it, a wrong or missed tap is orders of magnitude outside.

Also: exact integers, determinism (calls, a sliced batch, a graph replay), a NaN guard band, argument checks, the
StridedConv3x3BiasAct module inside the copies (paths, switches, refusals), whole-backbone accuracy against an fp64
forward, the loader and the API, and a copy with every f32 option on that calls no library convolution or GEMM."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cases

pytestmark = pytest.mark.gpu

ACTS = [None, 'relu', 'silu', 'hardswish']
_TORCH_ACT = {None: lambda t: t, 'relu': F.relu, 'silu': F.silu, 'hardswish': F.hardswish}


def _inputs(B, K, M, H, W, seed, residual, border=1.0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(B, K, H, W, device='cuda', generator=g)
    if border != 1.0:   # large border pixels: a wrong halo (a missed or a doubled edge tap) shows
        edge = torch.ones(H, W, device='cuda')
        edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = border
        x = x * edge
    w = torch.randn(M, K, 3, 3, device='cuda', generator=g) / (9 * K) ** 0.5
    b = 0.5 * torch.randn(M, device='cuda', generator=g)
    r = torch.randn(B, M, H // 2, W // 2, device='cuda', generator=g) if residual else None
    return x, w, b, r


def _ref64(x, w, b, act, r):
    ref = _TORCH_ACT[act](F.conv2d(x.double(), w.double(), b.double(), 2, 1))
    return ref if r is None else ref + r.double()


def _reference(x, w, b, act, r):
    """(fp64 result, the bound of the module docstring)."""
    K = x.shape[1]
    ref = _ref64(x, w, b, act, r)
    S = F.conv2d(x.double().abs(), w.double().abs(), None, 2, 1) + b.double().abs()[None, :, None, None]
    return ref, 1.1 * (9 * K + 2) * 2.0 ** -24 * S + 1e-6 * ref.abs() + 2.0 ** -24


def _check(x, w, b, act, r, got):
    """The bound of the module docstring, on every element (tests/conv_fuzz.py uses the same two functions)."""
    ref, bound = _reference(x, w, b, act, r)
    assert got.shape == ref.shape and got.dtype == torch.float32
    err = (got.double() - ref).abs()
    print(f'k22 check {tuple(x.shape)} -> {tuple(got.shape)} {act} skip {r is not None}: '
          f'max err / bound = {float((err / bound).max()):.4f}')
    excess = float((err - bound).max())
    assert excess <= 0, excess


def _run(x, w, b, act, r, **kw):
    from metrabs_amd import kernels
    wp = kernels.pack_conv3x3_strided_weight(w)
    assert kernels.conv3x3_strided_supported(x, wp), tuple(x.shape)
    return kernels.conv3x3_strided_bias_act(x, wp, b, act, residual=r, **kw)


# (B, Cin, Cout, H, W, the activation that runs with the skip): one partial tile, one k step, Cout below a fragment;
# tiles of several images, H != W; OW = 36, a partial position fragment, Cin no multiple of 8; Cout past a channel
# block's 128, OH = 4; OW = 4, a tall plane; OW = 96 (three tiles of two fragments) and Cout = 260: three channel blocks
EDGE_CASES = [(1, 4, 5, 8, 8, None), (3, 24, 96, 16, 24, 'relu'), (2, 12, 40, 40, 72, 'silu'),
              (2, 64, 130, 8, 16, 'hardswish'), (1, 8, 16, 72, 8, 'silu'), (1, 4, 260, 4, 192, 'relu')]


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('case', EDGE_CASES)
def test_k22_every_epilogue_and_edge_geometry(act, case, hip_lib):
    """The four activations on every geometry; the skip on once and off three times per geometry."""
    B, K, M, H, W, skip_act = case
    x, w, b, r = _inputs(B, K, M, H, W, 7, act == skip_act, border=8.0)
    _check(x, w, b, act, r, _run(x, w, b, act, r))


@functools.lru_cache(maxsize=None)
def _armed_shapes(name, res):
    """(Cin, Cout, H, W, act, residual) of every armed layer's input at `res` px, from a hooked forward."""
    from metrabs_amd import backbones
    S3 = backbones.StridedConv3x3BiasAct
    net = backbones.fold_batchnorm(backbones.build_backbone(name).eval(), fused_epilogue=True, strided3x3=True).cuda()
    shapes = set()

    def hook(mod, args, kwargs):
        x = args[0]
        shapes.add((x.shape[1], mod.conv.out_channels, x.shape[2], x.shape[3], mod.act_name,
                    kwargs.get('residual') is not None))

    hs = [m.register_forward_pre_hook(hook, with_kwargs=True) for m in net.modules() if isinstance(m, S3)]
    assert hs
    S3.use_k22 = False
    try:
        with torch.inference_mode():
            net(torch.rand(1, 3, res, res, device='cuda'))
    finally:
        S3.use_k22 = True
    for h in hs:
        h.remove()
    return tuple(sorted(shapes, key=str))


@pytest.mark.parametrize('name,res,count', [('efficientnetv2-s', 256, 2), ('efficientnetv2-s', 224, 2),
                                            ('efficientnetv2-l', 384, 2), ('resnet18', 256, 3)])
def test_k22_matches_fp64_on_every_armed_shape(name, res, count, hip_lib):
    shapes = _armed_shapes(name, res)
    assert len(shapes) == count, shapes
    for i, (K, M, H, W, act, res_) in enumerate(shapes):
        x, w, b, r = _inputs(1, K, M, H, W, 2000 + i, res_)
        _check(x, w, b, act, r, _run(x, w, b, act, r))


@pytest.mark.parametrize('skip', [False, True])
@pytest.mark.parametrize('shape', [(2, 24, 96, 16, 16), (1, 64, 256, 8, 8)])
def test_k22_is_exact_on_small_integers(shape, skip, hip_lib):
    """x in -3 .. 3, w in -2 .. 2, an integer bias and skip: every product and partial sum is an integer below 2^24
    (<= 9 * 64 * 6), so the fma chain is exact and the result must equal the fp64 convolution -- a swapped tap, a
    transposed fragment or a wrong halo cannot hide in rounding.  The weights have no symmetry in ky, kx, ci or m."""
    B, K, M, H, W = shape
    g = torch.Generator(device='cuda').manual_seed(3)
    x = torch.randint(-3, 4, (B, K, H, W), device='cuda', generator=g).float()
    w = torch.randint(-2, 3, (M, K, 3, 3), device='cuda', generator=g).float()
    b = (torch.arange(M, device='cuda') % 7 - 3).float()
    r = torch.randint(-9, 10, (B, M, H // 2, W // 2), device='cuda', generator=g).float() if skip else None
    ref = _ref64(x, w, b, None, r)
    assert float(ref.abs().max()) < 2 ** 24
    assert torch.equal(_run(x, w, b, None, r), ref.float())


def test_k22_is_deterministic_and_graph_safe(hip_lib):
    from metrabs_amd import kernels
    for (B, K, M, H, W, res_) in [(3, 24, 96, 32, 32, True), (3, 48, 192, 16, 16, False), (3, 12, 40, 40, 72, True)]:
        x, w, b, r = _inputs(B, K, M, H, W, 3, res_)
        wp = kernels.pack_conv3x3_strided_weight(w)
        a = kernels.conv3x3_strided_bias_act(x, wp, b, 'silu', residual=r)
        assert torch.equal(a, kernels.conv3x3_strided_bias_act(x, wp, b, 'silu', residual=r))
        # image 1 of 3 as a batch of its own: other workgroups, the same bits
        part = kernels.conv3x3_strided_bias_act(x[1:2], wp, b, 'silu', residual=None if r is None else r[1:2])
        assert torch.equal(part, a[1:2])
        with torch.inference_mode():
            out = torch.empty_like(a)
            assert kernels.conv3x3_strided_bias_act(x, wp, b, 'silu', residual=r, out=out) is out
            assert torch.equal(out, a)
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                kernels.conv3x3_strided_bias_act(x, wp, b, 'silu', residual=r, out=out)
                st.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                    kernels.conv3x3_strided_bias_act(x, wp, b, 'silu', residual=r, out=out)
            torch.cuda.current_stream().wait_stream(st)
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, a)


@pytest.mark.parametrize('shape', [(4, 5, 8, 8), (12, 40, 40, 72), (64, 130, 8, 16)])
def test_k22_writes_nothing_outside_y_and_reads_nothing_outside_its_inputs(shape, hip_lib):
    """x, y and the skip are carved out of one larger buffer filled with NaN: nothing outside y changes, no NaN gets
    into y (a read outside x or the skip that reached a stored value would bring one in), and y passes the bound."""
    from metrabs_amd import kernels
    K, M, H, W = shape
    B = 3
    x0, w, b, r0 = _inputs(B, K, M, H, W, 5, True, border=8.0)
    nx, ny, gap = x0.numel(), r0.numel(), 1024
    buf = torch.full((4 * gap + nx + 2 * ny,), float('nan'), device='cuda')
    ox, orr, oy = gap, 2 * gap + nx, 3 * gap + nx + ny
    x, r, y = buf[ox:ox + nx].view_as(x0), buf[orr:orr + ny].view_as(r0), buf[oy:oy + ny].view_as(r0)
    x.copy_(x0), r.copy_(r0)
    before = buf.view(torch.int32).clone()
    wp = kernels.pack_conv3x3_strided_weight(w)
    assert kernels.conv3x3_strided_bias_act(x, wp, b, 'relu', residual=r, out=y) is y
    torch.cuda.synchronize()
    after = buf.view(torch.int32)
    assert torch.equal(after[:oy], before[:oy]) and torch.equal(after[oy + ny:], before[oy + ny:])
    assert not torch.isnan(y).any()
    _check(x0, w, b, 'relu', r0, y)
    assert torch.equal(y, kernels.conv3x3_strided_bias_act(x0, wp, b, 'relu', residual=r0))


def test_k22_wrapper_argument_checks(hip_lib):
    from metrabs_amd import kernels
    x, w, b, r = _inputs(2, 8, 16, 16, 16, 1, True)
    wp = kernels.pack_conv3x3_strided_weight(w)
    ok = kernels.conv3x3_strided_bias_act(x, wp, b, None, residual=r)
    with pytest.raises(ValueError):
        kernels.conv3x3_strided_bias_act(x.half(), wp, b, None)                        # dtype
    with pytest.raises(ValueError):
        kernels.conv3x3_strided_bias_act(x, wp.half(), b, None)
    with pytest.raises(ValueError):
        kernels.conv3x3_strided_bias_act(x.to(memory_format=torch.channels_last), wp, b, None)   # layout
    with pytest.raises(ValueError):
        kernels.conv3x3_strided_bias_act(x, w, b, None)                                # the OIHW weight
    with pytest.raises(ValueError):
        kernels.conv3x3_strided_bias_act(x, wp[:1].contiguous(), b, None)              # another Cin
    with pytest.raises(ValueError):
        kernels.conv3x3_strided_bias_act(x, wp, b[:4], None)
    with pytest.raises(ValueError):
        kernels.conv3x3_strided_bias_act(x, wp, b, None, residual=r[:, :, :4].contiguous())
    with pytest.raises(ValueError):
        kernels.conv3x3_strided_bias_act(x, wp, b, None, residual=r.half())
    with pytest.raises(ValueError):                                                    # the input's size, not the output's
        kernels.conv3x3_strided_bias_act(x, wp, b, None, out=torch.empty(2, 16, 16, 16, device='cuda'))
    with pytest.raises(ValueError):
        kernels.conv3x3_strided_bias_act(x, wp, b, None, residual=r, out=r)            # an aliasing out
    flat = torch.zeros(x.numel() + 64, device='cuda')
    x_in = flat[:x.numel()].view_as(x)
    with pytest.raises(ValueError):                                                    # out inside x's storage
        kernels.conv3x3_strided_bias_act(x_in, wp, b, None, out=flat[64:64 + ok.numel()].view_as(ok))
    with pytest.raises(ValueError):
        kernels.conv3x3_strided_bias_act(x[:, :, :7].contiguous(), wp, b, None)        # odd H
    with pytest.raises(RuntimeError):                                                  # no CPU fallback
        kernels.conv3x3_strided_bias_act(x.cpu(), wp.cpu(), b.cpu(), None)
    with pytest.raises(RuntimeError):                                                  # MTR_E_SHAPE through check()
        kernels.conv3x3_strided_bias_act(x[:, :, :, :12].contiguous(), wp, b, None)
    assert kernels.conv3x3_strided_supported(x, wp)
    assert not kernels.conv3x3_strided_supported(x[:, :, :7].contiguous(), wp)         # odd H
    assert not kernels.conv3x3_strided_supported(x[:, :, :, :12].contiguous(), wp)     # (W / 2) % 4 != 0
    assert not kernels.conv3x3_strided_supported(x.to(memory_format=torch.channels_last), wp)
    assert not kernels.conv3x3_strided_supported(x.half(), wp.half())
    assert not kernels.conv3x3_strided_supported(x, w)
    flat = torch.zeros(x.numel() + 2, device='cuda')
    assert not kernels.conv3x3_strided_supported(flat[2:].view_as(x), wp)              # 8 bytes past a boundary
    assert torch.equal(ok, kernels.conv3x3_strided_bias_act(x, wp, b, None, residual=r))


def _calibrated(name, res, batch_size=4):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    return backbones.calibrate_batchnorm(backbones.build_backbone(name).cuda(), res, 'cuda', batch_size=batch_size)


def _pinned():
    return torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True)


def _all_paths(net):
    return [getattr(m, 'last_path', None) for m in net.modules()]


@functools.lru_cache(maxsize=None)
def _effnet_s_128():
    """One calibrated EfficientNetV2-S, its default and armed folded copies, an input, the default copy's features under
    the deterministic pin and the fp64 CPU forward of the same folded network: made once, left unchanged."""
    import copy
    from metrabs_amd import backbones
    net = _calibrated('efficientnetv2-s', 128)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, strided3x3=True)
    x = torch.rand(2, 3, 128, 128, device='cuda', generator=torch.Generator(device='cuda').manual_seed(4))
    with torch.inference_mode():
        want = copy.deepcopy(plain).cpu().double()(x.cpu().double())
        with _pinned():
            ref = plain(x).clone()
    return plain, armed, x, ref, want


def test_armed_efficientnet_takes_k22_where_it_applies(hip_lib):
    from metrabs_amd import backbones
    S3 = backbones.StridedConv3x3BiasAct
    plain, armed, x, ref, _ = _effnet_s_128()
    feats = armed[1]
    mods = [m for m in armed.modules() if isinstance(m, S3)]
    assert len(mods) == 2 and 'k22' not in _all_paths(plain)
    with torch.inference_mode(), _pinned():
        on = armed(x).clone()
        assert [m.last_path for m in mods] == ['k22', 'k22']
        for stage in (feats[2], feats[3]):                # stages 2 - 3: the stride-2 first block, then stride-1 blocks
            assert stage[0].last_path == 'k22' and stage[0].pre_pair[0] in mods
            assert stage[0].pre_pair[1].last_path == 'k13'
            assert all(blk.last_path == 'k13_pre' for blk in list(stage)[1:])
        assert torch.isfinite(on).all() and not torch.equal(on, ref)
        rel = float((on - ref).norm() / ref.norm())
        print(f'armed vs default copy, EfficientNetV2-S 128 px: relative difference {rel:.3g}')
        assert rel < 1e-4
        # the switch, and a listed shape: exactly what the default copy runs, the same bits
        shipped = S3.k22_slower
        try:
            S3.use_k22 = False
            off = armed(x).clone()
            assert all(m.last_path == 'library' for m in mods) and 'k22' not in _all_paths(armed)
            assert feats[2][0].last_path == 'k13_pre' and feats[3][0].last_path == 'k13_pre'
            assert torch.equal(off, ref)
            S3.use_k22 = True
            S3.k22_slower = frozenset({(24, 96, 64, 64)})
            armed(x)
            assert feats[2][0].last_path == 'k13_pre' and feats[3][0].last_path == 'k22'
        finally:
            S3.use_k22, S3.k22_slower = True, shipped
        # autocast and a channels_last input: the library path
        with torch.autocast('cuda', dtype=torch.float16):
            armed(x)
        assert all(m.last_path == 'library' for m in mods)
        armed(x)
        assert all(m.last_path == 'k22' for m in mods)
        m0 = mods[0]
        xin = torch.rand(2, 24, 64, 64, device='cuda')
        assert m0.k22_takes(xin) and not m0.k22_takes(xin.to(memory_format=torch.channels_last))
        assert m0.path(xin) == 'k22' and m0.path(xin.to(memory_format=torch.channels_last)) == 'library'
        m0(xin.to(memory_format=torch.channels_last))
        assert m0.last_path == 'library'
        m0(xin)
        assert m0.last_path == 'k22'
        assert not m0.k22_takes(xin[:, :, :63, :63].contiguous())                      # an odd map
    xg = torch.rand(2, 24, 64, 64, device='cuda', requires_grad=True)   # a gradient wanted: the library path
    assert not mods[0].k22_takes(xg) and mods[0].path(xg) == 'library'


def test_armed_resnet18_takes_k22_on_its_three_layers(hip_lib):
    from metrabs_amd import backbones
    S3 = backbones.StridedConv3x3BiasAct
    net = _calibrated('resnet18', 128)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, strided3x3=True)
    mods = [m for m in armed.modules() if isinstance(m, S3)]
    assert len(mods) == 3
    x = torch.rand(2, 3, 256, 256, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    with torch.inference_mode(), _pinned():
        y, ref = armed(x), plain(x)
    assert torch.isfinite(y).all()
    assert [m.last_path for m in mods] == ['k22'] * 3
    assert float((y - ref).norm() / ref.norm()) < 1e-4


def test_whole_backbone_accuracy_against_fp64(hip_lib):
    """The armed copy's features against an fp64 CPU forward of the same folded network: a relative RMS error of at
    most 2 x the default copy's (the parent's path) against that same forward -- both are rounding noise from
    different summation orders, hence the margin (the criterion of DESIGN.md sections 22 - 24)."""
    plain, armed, x, ref, want = _effnet_s_128()
    with torch.inference_mode(), _pinned():
        got_armed = armed(x).double().cpu()
    assert 'k22' in _all_paths(armed)
    rel = lambda t: float((t - want).norm() / want.norm())
    e_plain, e_armed = rel(ref.double().cpu()), rel(got_armed)
    print(f'efficientnetv2-s 128 px B = 2, relative RMS error against fp64: default copy {e_plain:.4g}, '
          f'armed copy {e_armed:.4g}')
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


def _poses(est, images, boxes, num_aug=1):
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


def test_k22_through_the_loader_and_the_api(tmp_path, hip_lib):
    """Three crops through estimate_poses_batched.  A graphed call of the armed model returns the eager call's bits, and
    MPJPE(armed, fp64) <= 2 x MPJPE(default copy, fp64), the reference being the same folded network with its backbone
    evaluated in fp64 on the CPU (sampler and head are the same kernels for every arm): both are f32 rounding noise
    from different summation orders.  A wrong armed layer moves the features by far more."""
    from metrabs_amd import backbones, loading
    d = _model_dir(tmp_path)
    plain = loading.load_multiperson_model(d, fold_batchnorm=True, fused_epilogue=True)
    truth = loading.load_multiperson_model(d, fold_batchnorm=True, fused_epilogue=True)
    truth.crop_model.backbone = _Fp64Backbone(truth.crop_model.backbone)
    est = loading.load_multiperson_model(d, strided3x3=True)
    eager = loading.load_multiperson_model(d, strided3x3=True)
    for m in (plain, est, eager):
        m.crop_model.deterministic_backbone = True
    est.graph_batches, eager.graph_batches, truth.graph_batches = True, False, False
    images, boxes = _api_inputs(5)
    p_armed, p_graph = _poses(eager, images, boxes), _poses(est, images, boxes)
    assert torch.isfinite(p_armed).all()
    assert torch.equal(p_armed, p_graph), float((p_armed - p_graph).abs().max())
    for model in (est, eager):
        paths = [m.last_path for m in model.crop_model.backbone.modules()
                 if isinstance(m, backbones.StridedConv3x3BiasAct)]
        assert paths == ['k22'] * 2, paths
    p_true, p_plain = _poses(truth, images, boxes), _poses(plain, images, boxes)
    assert 'k22' not in _all_paths(plain.crop_model.backbone)
    assert p_true.shape == p_armed.shape and torch.isfinite(p_true).all()
    mpjpe = lambda p, q: float((p - q).norm(dim=-1).mean())
    e_armed, e_plain = mpjpe(p_armed, p_true), mpjpe(p_plain, p_true)
    print(f'MPJPE to the fp64-backbone poses: armed copy {e_armed:.5g} mm, default copy {e_plain:.5g} mm; '
          f'mean |p| {float(p_true.norm(dim=-1).mean()):.4g} mm')
    assert 0 < e_armed <= 2 * e_plain, (e_armed, e_plain)


def _op_names(net, x):
    from torch.utils._python_dispatch import TorchDispatchMode

    class Record(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.names = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.names.append(str(func))
            return func(*args, **(kwargs or {}))

    with torch.inference_mode(), Record() as rec:
        y = net(x)
    return y, rec.names


def test_no_library_convolution_is_left_with_every_f32_option_on(hip_lib):
    """EfficientNetV2-S at 256 px, B = 2, folded with fuse_stem, block_depthwise, winograd3x3, split_gemm and strided3x3,
    WITHOUT the deterministic-solver pin: no ATen convolution, matrix product or linear is dispatched during the forward
    (with K22 switched off at least one convolution is), every module with a last_path reports a hand-written kernel,
    and two forwards and a graph replay return the same bits."""
    from metrabs_amd import backbones
    S3 = backbones.StridedConv3x3BiasAct
    net = _calibrated('efficientnetv2-s', 256)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, fuse_stem=True, block_depthwise=True, winograd3x3=True,
                                     split_gemm=True, strided3x3=True)
    x = torch.rand(2, 3, 256, 256, device='cuda', generator=torch.Generator(device='cuda').manual_seed(2))
    # (under inference_mode a convolution is dispatched as aten.conv2d, not decomposed to aten.convolution: 'conv' matches
    # both, and whatever else the library might be reached through)
    library = lambda names: [n for n in names if any(k in n for k in ('conv', 'mm', 'linear'))]
    shipped = S3.k22_slower
    try:
        S3.k22_slower = frozenset()
        y, names = _op_names(armed, x)
        assert library(names) == [], library(names)
        paths = [p for p in _all_paths(armed) if p is not None]
        assert paths and 'library' not in paths and paths.count('k22') == 4   # two layers, their two blocks
        with torch.inference_mode():
            assert torch.isfinite(y).all() and torch.equal(armed(x), y)
            static = x.clone()
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                armed(static)
                st.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                    out = armed(static)
            torch.cuda.current_stream().wait_stream(st)
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, y)
        S3.use_k22 = False
        _, names_off = _op_names(armed, x)
        assert any('conv' in n for n in names_off), names_off
    finally:
        S3.use_k22, S3.k22_slower = True, shipped

"""GPU: K15 (csrc/depthwise5x5.hip, kernels.depthwise5x5_bias_act) -- depthwise 5x5 + bias + activation (+ the
plane mean) in one pass -- against fp64, exactly on integers, path against path bit for bit, inside the folded
MobileNetV3 and through the API with HIP graphs.

The accuracy bound (no free tolerance).  Inputs are rounded to the tensor's dtype first, weights and bias are
f32, so every product x*w the kernel forms has the fp64 reference's operands.  With u = 2^-24:
  * pre-activation v: 25 fma and one addition of the bias, each one f32 rounding of a partial sum that is at
    most S = sum |x*w| + |b| in magnitude: |v_hat - v| <= gamma_26 S < 27 u S (Higham, Accuracy and Stability,
    eq. 3.7 applied to the fma chain);
  * the activation is Lipschitz with constant L <= 1.5 (hardswish: (2x + 3) / 6 at x = 3; silu 1.1, relu and none
    1), which carries that error to 1.5 * 27 u S, and is itself evaluated in f32: hardswish is an addition, a clamp,
    two products and the rounded constant 1/6 (5 roundings); silu is x * rcp(1 + exp2(-x log2 e)), where the
    rounded argument of exp2 costs 2 |v| u relative and v_exp_f32, the addition, v_rcp_f32 (1 ulp = 2 u each)
    and the product 6 u more: together at most (8 + 2 |v|) u |act(v)|;
  * one rounding to the output dtype: u_out |y_hat| with u_out = 2^-24 (f32), 2^-11 (f16), 2^-8 (bf16), plus
    half the smallest subnormal for f16 (2^-25).
  bound = E (1 + u_out) + u_out |act(v)| + tiny,   E = 1.5 * 27 u S + (8 + 2 |v|) u |act(v)|
Each test prints the largest observed error as a share of this bound."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _leave_the_device_idle():
    """Nothing of a test here outlives it on the GPU: the graphs, side streams and static buffers of the estimators and
    the captured graphs are collected and every stream has drained before the next test's first allocation."""
    yield
    import gc
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
ACTS = [None, 'relu', 'silu', 'hardswish']
U_OUT = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
# MobileNetV3-Large's 5x5 layers: (C, stride, activation), input map = res / MAP_DIV
MBV3_5X5 = [(72, 2, 'relu', 4), (120, 1, 'relu', 8), (672, 2, 'hardswish', 16), (960, 1, 'hardswish', 32)]


def _act64(v, act):
    if act == 'relu':
        return v.clamp_min(0)
    if act == 'silu':
        return v * torch.sigmoid(v)
    if act == 'hardswish':
        return v * (v + 3).clamp(0, 6) / 6
    return v


def _inputs(B, C, H, W, dtype, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(B, C, H, W, device='cuda', generator=g).to(dtype)   # rounded to the tensor dtype first
    w = torch.randn(C, 1, 5, 5, device='cuda', generator=g) * 0.3
    b = torch.randn(C, device='cuda', generator=g)
    return x, w, b


def _pads(pad):
    return (pad,) * 4 if isinstance(pad, int) else tuple(pad)   # (left, right, top, bottom)


def _reference(x, w, b, act, stride, pad):
    """fp64: (act(v), v, S) with S = sum |x w| + |b|."""
    xd = F.pad(x.double(), _pads(pad))
    C = x.shape[1]
    v = F.conv2d(xd, w.double(), b.double(), stride, 0, groups=C)
    S = F.conv2d(xd.abs(), w.double().abs(), b.double().abs(), stride, 0, groups=C)
    return _act64(v, act), v, S


def _ref_and_bound(x, w, b, act, stride, pad):
    """(fp64 result, the bound of the module docstring): what _check compares y with (tests/conv_fuzz.py)."""
    ref, v, S = _reference(x, w, b, act, stride, pad)
    u, uo = 2.0 ** -24, U_OUT[x.dtype]
    E = 1.5 * 27 * u * S + (8 + 2 * v.abs()) * u * ref.abs()
    return ref, E * (1 + uo) + uo * ref.abs() + 2.0 ** -25


def _check(x, w, b, act, stride, pad, y, mean=None, tag=''):
    ref, bound = _ref_and_bound(x, w, b, act, stride, pad)
    assert y.shape == ref.shape and y.dtype == x.dtype
    u = 2.0 ** -24
    err = (y.double() - ref).abs()
    share = float((err / bound).max())
    print(f'[k15] {tag} {tuple(x.shape)} {str(x.dtype)[6:]} act={act} s={stride} pad={pad}: '
          f'max err {float(err.max()):.3e}, largest share of the bound {share:.3f}')
    assert share <= 1.0, (tag, share)
    if mean is not None:
        # f32 sum of n = OH * OW rounded outputs, then one product: |err| <= (n + 1) u sum |y| / n
        n = y.shape[2] * y.shape[3]
        want = y.double().mean((2, 3))
        mbound = (n + 1) * u * y.double().abs().mean((2, 3)) + 2.0 ** -126
        mshare = float(((mean.double() - want).abs() / mbound).max())
        print(f'[k15] {tag} mean: largest share of the summation bound {mshare:.3f}')
        assert mean.shape == want.shape and mean.dtype == torch.float32 and mshare <= 1.0, (tag, mshare)
    return share


def _largest_batch(C, OH, OW):
    """64 or 320, whichever is the largest whose fp64 reference stays below 2^26 outputs."""
    return 320 if 320 * C * OH * OW < 2 ** 26 else 64


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C,stride,act,div', MBV3_5X5)
def test_mobilenetv3_shapes_match_fp64(C, stride, act, div, dtype, hip_lib):
    from metrabs_amd import kernels
    H = 256 // div
    for B in (1, 3, _largest_batch(C, H // stride, H // stride)):
        x, w, b = _inputs(B, C, H, H, dtype, 100 + B)
        y, mean = kernels.depthwise5x5_bias_act(x, w, b, act, stride, 2, want_mean=True)
        _check(x, w, b, act, stride, 2, y, mean, tag=f'mbv3@256 B={B}')
        assert torch.equal(y, kernels.depthwise5x5_bias_act(x, w, b, act, stride, 2))  # same bits without the mean


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('res', [224, 160, 128])
def test_eligible_shapes_at_other_resolutions(res, dtype, hip_lib):
    from metrabs_amd import kernels
    ran = 0
    for C, stride, act, div in MBV3_5X5:
        H = res // div
        if ((H + 4 - 5) // stride + 1) % 4:
            continue   # 14 -> 7 and 7x7 at 224 px, 10 -> 5 and 5x5 at 160 px: the module's library path
        x, w, b = _inputs(5, C, H, H, dtype, res + C)
        y, mean = kernels.depthwise5x5_bias_act(x, w, b, act, stride, 2, want_mean=True)
        _check(x, w, b, act, stride, 2, y, mean, tag=f'mbv3@{res}')
        ran += 1
    assert ran == {224: 2, 160: 2, 128: 4}[res]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('act', ACTS)
def test_paddings_odd_planes_and_ragged_plane_counts(act, dtype, hip_lib):
    from metrabs_amd import kernels
    cases = [  # (B, C, H, W, stride, pad (left, right, top, bottom))
        (2, 7, 16, 16, 2, (2, 2, 2, 2)), (2, 5, 16, 16, 2, (1, 3, 1, 3)), (3, 1, 32, 32, 2, (1, 3, 1, 3)),
        (2, 5, 9, 12, 1, 2), (1, 7, 13, 20, 1, 2), (2, 1, 6, 24, 1, 2), (1, 5, 11, 40, 1, 2),
        (2, 5, 15, 24, 2, (2, 2, 2, 2)), (1, 7, 21, 40, 2, (1, 3, 1, 3)), (2, 1, 7, 12, 1, (2, 2, 1, 3)),
        (70, 3, 8, 8, 1, 2), (70, 3, 16, 16, 2, (1, 3, 1, 3)), (70, 3, 32, 32, 1, 2),   # a last group that is not full
        (1, 5, 20, 20, 1, 0), (1, 5, 19, 19, 2, (0, 0, 0, 0)), (2, 3, 10, 12, 1, (0, 0, 2, 3)),
        (1, 2, 100, 108, 1, 2), (1, 2, 108, 104, 2, 2),   # the largest planes the entry takes
    ]
    for i, (B, C, H, W, stride, pad) in enumerate(cases):
        x, w, b = _inputs(B, C, H, W, dtype, 300 + i)
        y, mean = kernels.depthwise5x5_bias_act(x, w, b, act, stride, pad, want_mean=True)
        _check(x, w, b, act, stride, pad, y, mean, tag=f'case {i}')
        assert torch.equal(y, kernels.depthwise5x5_bias_act(x, w, b, act, stride, pad))


# taps 0 .. 24 in row-major order, minus 12: different at every tap, asymmetric in both axes
_TAPS = (torch.arange(25, dtype=torch.float32) - 12.0).view(1, 1, 5, 5)


def _exact_case(B, C, H, W, seed):
    """Integers in -1 .. 1 inside the plane and in -2 .. 2 (twice as large) on its border rows and columns, taps
    -12 .. 12 with the sign flipped on every other channel, an integer bias: every product, partial sum and output
    is a small integer, exact in f32.  The worst case is 2 * 156 + 3 = 315; bf16 holds integers exactly up to 256, so
    the caller checks on the CPU that the outputs of the seeds used stay within 256 (and reach 64)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-1, 2, (B, C, H, W), generator=g).float()
    edge = torch.randint(-2, 3, (B, C, H, W), generator=g).float()
    border = torch.zeros(H, W, dtype=torch.bool)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    x = torch.where(border, edge, x)
    w = _TAPS.repeat(C, 1, 1, 1) * torch.tensor([1.0, -1.0]).repeat((C + 1) // 2)[:C].view(C, 1, 1, 1)
    b = torch.arange(C, dtype=torch.float32) - C // 2
    return x, w, b


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('stride,pad', [(1, 2), (2, 2), (2, (1, 3, 1, 3)), (1, (2, 2, 1, 3)), (2, (0, 3, 2, 1))])
def test_exact_on_integers(stride, pad, dtype, hip_lib):
    from metrabs_amd import kernels
    ran = 0
    for H, W in [(8, 8), (16, 16), (13, 24)]:
        x, w, b = _exact_case(3, 6, H, W, 7 * H + W)
        want = F.conv2d(F.pad(x.double(), _pads(pad)), w.double(), b.double(), stride, 0, groups=6)
        if want.shape[3] % 4:
            continue
        assert float(want.abs().max()) <= 256 and float(want.abs().max()) >= 64   # exact in bf16, and not trivial
        assert torch.equal(want, want.round())
        y, mean = kernels.depthwise5x5_bias_act(x.cuda().to(dtype), w.cuda(), b.cuda(), None, stride, pad,
                                                want_mean=True)
        assert torch.equal(y.double().cpu(), want), (H, W, float((y.double().cpu() - want).abs().max()))
        ran += 1
    assert ran >= 2


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C,H,stride,pad,act', [(72, 64, 2, 2, 'relu'), (120, 32, 1, 2, 'relu'),
                                                (672, 16, 2, (1, 3, 1, 3), 'hardswish'), (960, 8, 1, 2, 'hardswish'),
                                                (5, 13, 1, 2, 'silu')])
def test_every_path_gives_the_same_bits(C, H, stride, pad, act, dtype, hip_lib):
    """Aligned base (vector rows) against a base one element further (scalar rows); call against call; a captured
    HIP graph replayed twice against the eager call."""
    from metrabs_amd import kernels
    W = H if H % 4 == 0 else 20
    x, w, b = _inputs(6, C, H, W, dtype, 500 + C)
    assert x.data_ptr() % 16 == 0
    y, mean = kernels.depthwise5x5_bias_act(x, w, b, act, stride, pad, want_mean=True)
    _check(x, w, b, act, stride, pad, y, mean, tag='paths')
    buf = torch.zeros(x.numel() + 8, device='cuda', dtype=dtype)
    shifted = buf[1:1 + x.numel()].view_as(x)
    shifted.copy_(x)
    assert shifted.is_contiguous() and shifted.data_ptr() % (4 * x.element_size()) != 0
    y2, mean2 = kernels.depthwise5x5_bias_act(shifted, w, b, act, stride, pad, want_mean=True)
    assert torch.equal(y, y2) and torch.equal(mean, mean2)
    y3, mean3 = kernels.depthwise5x5_bias_act(x, w, b, act, stride, pad, want_mean=True)
    assert torch.equal(y, y3) and torch.equal(mean, mean3)
    with torch.inference_mode():
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            kernels.depthwise5x5_bias_act(x, w, b, act, stride, pad, want_mean=True)
            st.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                gy, gmean = kernels.depthwise5x5_bias_act(x, w, b, act, stride, pad, want_mean=True)
        torch.cuda.current_stream().wait_stream(st)
        for _ in range(2):
            gy.zero_()
            gmean.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(gy, y) and torch.equal(gmean, mean)


def test_wrapper_and_entry_refuse_what_k15_does_not_take(hip_lib):
    from metrabs_amd import kernels
    x, w, b = _inputs(1, 4, 16, 16, torch.float32, 1)
    with pytest.raises(ValueError):
        kernels.depthwise5x5_bias_act(x, w[:, :, :3, :3].contiguous(), b, None, 1, 2)   # a 3x3 weight
    with pytest.raises(ValueError):
        kernels.depthwise5x5_bias_act(x.transpose(2, 3), w, b, None, 1, 2)
    with pytest.raises(RuntimeError):
        kernels.depthwise5x5_bias_act(x, w, b, None, 3, 2)
    with pytest.raises(RuntimeError):
        kernels.depthwise5x5_bias_act(x[..., :14].contiguous(), w, b, None, 1, 2)       # OW = 14
    with pytest.raises(RuntimeError):
        kernels.depthwise5x5_bias_act(x, w, b, None, 1, (3, 2, 2, 2))
    assert not kernels.depthwise5x5_supported(128, 128, 2) and kernels.depthwise5x5_supported(108, 108, 2)


# ---- the module inside the folded network

def _calibrated(name, res, batch_size=4):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    return backbones.calibrate_batchnorm(backbones.build_backbone(name).cuda(), res, 'cuda', batch_size=batch_size)


def _five(net):
    from metrabs_amd import backbones
    return [m for m in net.modules() if isinstance(m, backbones.DepthwiseBiasAct) and m.k == 5]


def _count_se_gate(monkeypatch):
    from metrabs_amd import kernels
    calls = []
    orig = kernels.se_gate

    def counted(*a, **kw):
        calls.append(1)
        return orig(*a, **kw)

    monkeypatch.setattr(kernels, 'se_gate', counted)
    return calls


def _gates_16bit(a, b, c):
    """test_gpu_backbone16.test_copy_on_every_backbone's gates: a = f32 features, b = the f32 copy under autocast of
    the dtype, c = the 16-bit copy."""
    a = a.float()
    mean_c, mean_b = float((c.float() - a).abs().mean()), float((b.float() - a).abs().mean())
    amax = float(a.abs().max())
    assert mean_c <= 1.1 * mean_b + 1e-6 * amax, (mean_c, mean_b)
    max_c, max_b = float((c.float() - a).abs().max()), float((b.float() - a).abs().max())
    if max_b <= 0.1 * amax:
        assert max_c <= 0.1 * amax, (max_c, max_b, amax)
    else:
        assert max_c <= 1.1 * max_b, (max_c, max_b, amax)


@pytest.mark.parametrize('kernel_sizes', [(3, 5), (3,)])
def test_folded_mobilenetv3_runs_its_5x5_layers_on_k15(kernel_sizes, hip_lib, monkeypatch):
    from metrabs_amd import backbones
    monkeypatch.setattr(backbones.DepthwiseBiasAct, 'kernel_sizes', kernel_sizes)
    net = _calibrated('mobilenetv3', 256)
    n_se = sum(isinstance(m, backbones.SqueezeExcite) for m in net.modules())
    assert n_se == 8
    x = torch.rand(8, 3, 256, 256, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    with torch.inference_mode():
        want = net(x)
    f32 = backbones.fold_batchnorm(net, fused_epilogue=True)
    for dtype in (None, torch.float16, torch.bfloat16):
        copy = f32 if dtype is None else backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype)
        calls = _count_se_gate(monkeypatch)
        with torch.inference_mode():
            got = copy(x)
        assert len(calls) == n_se, (dtype, len(calls))   # once per squeeze-excite block: every mean arrived
        if kernel_sizes == (3, 5):
            five = _five(copy)
            assert len(five) == 6 and [m.last_path for m in five] == ['k15'] * 6
            assert all(m.last_path == 'k11' for m in copy.modules()
                       if isinstance(m, backbones.DepthwiseBiasAct) and m.k == 3)
        else:   # the tree and the path from before K15
            assert not _five(copy)
            five = [m for m in copy.modules() if isinstance(m, backbones.ConvBiasAct) and m.conv.kernel_size == (5, 5)]
            assert len(five) == 6 and all(isinstance(m.conv, backbones.DepthwiseConv2d) for m in five)
            assert [m.last_path for m in five] == ['library'] * 6
        if dtype is None:
            err = float((got - want).abs().max())
            print(f'[k15] folded mobilenetv3 f32 kernel_sizes={kernel_sizes}: {err / float(want.abs().max()):.2e} of max')
            assert err <= 1e-3 * float(want.abs().max())
        else:
            with torch.inference_mode(), torch.autocast('cuda', dtype=dtype):
                auto = f32(x)
            assert got.dtype == dtype
            _gates_16bit(want, auto, got)


def test_folded_mobilenetv3_at_224_px_leaves_the_odd_maps_to_the_library(hip_lib):
    from metrabs_amd import backbones
    net = _calibrated('mobilenetv3', 224)
    x = torch.rand(4, 3, 224, 224, device='cuda', generator=torch.Generator(device='cuda').manual_seed(2))
    for dtype in (None, torch.float16):
        copy = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype)
        with torch.inference_mode():
            want, got = net(x), copy(x)
        # 56 -> 28 and 28x28 on K15; 14 -> 7 and 7x7 (OW = 7) on the torch ops
        assert [m.last_path for m in _five(copy)] == ['k15'] * 3 + ['library'] * 3
        assert torch.isfinite(got).all()
        if dtype is None:
            assert float((got - want).abs().max()) <= 1e-3 * float(want.abs().max())


def test_k15_slower_sends_a_shape_to_the_library(hip_lib, monkeypatch):
    from metrabs_amd import backbones
    net = _calibrated('mobilenetv3', 256)
    x = torch.rand(2, 3, 256, 256, device='cuda', generator=torch.Generator(device='cuda').manual_seed(3))
    copy = backbones.fold_batchnorm(net, fused_epilogue=True)
    monkeypatch.setattr(backbones.DepthwiseBiasAct, 'k15_slower', frozenset({(960, 8, 8, 1)}))
    with torch.inference_mode():
        want, got = net(x), copy(x)
    assert [m.last_path for m in _five(copy)] == ['k15'] * 4 + ['library'] * 2
    assert float((got - want).abs().max()) <= 1e-3 * float(want.abs().max())


# ---- through the API, with HIP graphs

def _model_dir(tmp_path):
    import numpy as np
    from oracle import cases
    from metrabs_amd import loading
    from metrabs_amd.config import MetrabsConfig
    from metrabs_amd.joint_info import JointInfo
    from metrabs_amd.models.metrabs import Metrabs
    raw = dict(proc_side=256, stride_train=32, stride_test=32, centered_stride=True, depth=8,
               box_size_mm=2200, backbone='mobilenetv3', weak_perspective=False, mix_3d_inside_fov=0.5)
    bb = _calibrated('mobilenetv3', 256).cpu()
    torch.manual_seed(11)
    model = Metrabs(bb, JointInfo(cases.COCO17, cases.COCO17_EDGES), MetrabsConfig.from_any(raw),
                    in_channels=bb.out_channels)
    skel = {'': dict(indices=list(range(17)), names=cases.COCO17, edges=cases.COCO17_EDGES)}
    d = str(tmp_path / 'model')
    loading.save_model_dir(d, model, raw, skel, np.eye(17, dtype=np.float32))
    return d


def test_mobilenetv3_estimator_graphed_equals_eager(tmp_path, hip_lib):
    from oracle import cases
    from metrabs_amd import loading
    d = _model_dir(tmp_path)
    eager = loading.load_multiperson_model(d, fold_batchnorm=True, fused_epilogue=True)
    graphed = loading.load_multiperson_model(d, fold_batchnorm=True, fused_epilogue=True)
    for est in (eager, graphed):
        est.crop_model.deterministic_backbone = True   # the deterministic pin
        assert est.crop_model.backbone_is_pinned()
    eager.graph_batches = False
    graphed.graph_batches = True
    boxes = [torch.tensor([[60.0, 20.0, 120.0, 200.0], [150.0, 30.0, 100.0, 180.0]]),
             torch.tensor([[40.0, 10.0, 140.0, 210.0]])]
    for seed in (5, 9, 13):
        images = torch.stack([cases.synth_images(1, 240, 320, seed + i)[0] for i in range(2)]).cuda()
        with torch.inference_mode():
            a = torch.cat(eager.estimate_poses_batched(images, boxes, num_aug=5)['poses3d']).clone()
            b = torch.cat(graphed.estimate_poses_batched(images, boxes, num_aug=5)['poses3d']).clone()
        assert torch.isfinite(a).all() and float(a.abs().max()) > 0
        assert torch.equal(a, b), float((a - b).abs().max())
    for est in (eager, graphed):
        assert [m.last_path for m in _five(est.crop_model.backbone)] == ['k15'] * 6
    assert graphed.graphs.stats['captures'] >= 1 and graphed.graphs.stats['replays'] >= 1, graphed.graphs.stats
    assert eager.graphs.stats['captures'] == 0

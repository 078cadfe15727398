"""GPU: the 16-bit inference copy of the backbone (backbones.fold_batchnorm(dtype=)) and its 1x1 convolution
kernel K13h (csrc/conv1x1_16.hip): K13h against fp64 on every backbone shape, its epilogues, gate rounding,
determinism and argument checks; the copy on every backbone against the f32 network and f32 under autocast;
the copy through the loader and the drop-in API."""
import ctypes
import os

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


def _conv1x1_shapes(name, res):
    """(Cin, Cout, H, W, act, residual) of every 1x1 stride-1 ConvBiasAct of a folded backbone at `res` px."""
    from metrabs_amd import backbones
    net = backbones.fold_batchnorm(backbones.build_backbone(name).eval(), fused_epilogue=True).cuda()
    shapes = set()

    def hook(mod, args, kwargs):
        x = args[0]
        if mod.conv.kernel_size == (1, 1) and mod.conv.stride == (1, 1):
            shapes.add((x.shape[1], mod.conv.out_channels, x.shape[2], x.shape[3], mod.act_name,
                        kwargs.get('residual') is not None))

    hs = [m.register_forward_pre_hook(hook, with_kwargs=True) for m in net.modules()
          if isinstance(m, backbones.ConvBiasAct)]
    with torch.inference_mode():
        net(torch.rand(1, 3, res, res, device='cuda'))
    for h in hs:
        h.remove()
    return sorted(shapes, key=str)


def _inputs(B, K, M, H, W, seed, gate, residual, dtype):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(B, K, H, W, device='cuda', generator=g).to(dtype)
    w = (torch.randn(M, K, 1, 1, device='cuda', generator=g) / K ** 0.5).to(dtype)
    b = 0.5 * torch.randn(M, device='cuda', generator=g)
    gt = torch.rand(B, K, device='cuda', generator=g) if gate else None
    r = torch.randn(B, M, H, W, device='cuda', generator=g).to(dtype) if residual else None
    return x, w, b, gt, r


def _reference(x, w, b, act, gt, r):
    """(fp64 result, bound): |got - fp64| <= one unit in the last place of the 16-bit result + an f32-accumulation term
    ~ K 2^-24 sum_k |w xg| (through the activation, Lipschitz <= 1.1 here), where xg is torch's x * gate.to(x.dtype)
    and the fp64 sum runs over the 16-bit operands."""
    dt = x.dtype
    xg = x if gt is None else x * gt.to(dt)[:, :, None, None]
    wd = w.double().flatten(1)
    K = x.shape[1]
    z = torch.einsum('mk,bkhw->bmhw', wd, xg.double()) + b.double()[None, :, None, None]
    s = torch.einsum('mk,bkhw->bmhw', wd.abs(), xg.double().abs()) + b.double().abs()[None, :, None, None]
    ref = _TORCH_ACT[act](z)
    if r is not None:
        ref = ref + r.double()
    tiny = torch.finfo(dt).tiny
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(tiny))) - _MANT[dt])
    return ref, ulp + 1.1 * K * 2.0 ** -24 * s + 1e-6 * ref.abs() + 2.0 ** -24


def _check(x, w, b, act, gt, r, got):
    """_reference's bound on every element (tests/conv_fuzz.py uses the same two functions)."""
    ref, bound = _reference(x, w, b, act, gt, r)
    assert got.shape == ref.shape and got.dtype == x.dtype
    excess = float(((got.double() - ref).abs() - bound).max())
    assert excess <= 0, excess


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name,res', [('efficientnetv2-s', 256), ('efficientnetv2-l', 384), ('mobilenetv3', 256)])
@pytest.mark.parametrize('B', [1, 3, 64])
def test_k13h_matches_fp64_on_every_backbone_shape(name, res, B, dtype, hip_lib):
    from metrabs_amd import kernels
    shapes = _conv1x1_shapes(name, res)
    assert shapes
    for i, (K, M, H, W, act, res_) in enumerate(shapes):
        if B == 64 and H * W > 64 * 64 and K * M > 64 * 64:
            continue   # (the first layers at 128 px maps: covered at B = 1, 3)
        x, w, b, gt, r = _inputs(B, K, M, H, W, 1000 + i, i % 2 == 0, res_, dtype)
        assert kernels.conv1x1_16_supported(x, w)
        _check(x, w, b, act, gt, r, kernels.conv1x1_bias_act16(x, w, b, act, gate=gt, residual=r))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('gate', [False, True])
@pytest.mark.parametrize('residual', [False, True])
@pytest.mark.parametrize('shape', [(960, 160, 16, 16), (160, 960, 16, 16), (1536, 256, 8, 8), (64, 256, 32, 32),
                                   (24, 72, 12, 12), (200, 80, 4, 4), (40, 16, 8, 8)])
def test_k13h_every_epilogue(act, gate, residual, shape, dtype, hip_lib):
    from metrabs_amd import kernels
    K, M, H, W = shape
    x, w, b, gt, r = _inputs(3, K, M, H, W, 7, gate, residual, dtype)
    got = kernels.conv1x1_bias_act16(x, w, b, act, gate=gt, residual=r)
    _check(x, w, b, act, gt, r, got)
    if gate:   # the gate rounding rule: the staged x * g has exactly the bits of torch's x * g.to(x.dtype)
        pre = x * gt.to(dtype)[:, :, None, None]
        assert torch.equal(got, kernels.conv1x1_bias_act16(pre, w, b, act, residual=r))


@pytest.mark.parametrize('dtype', DTYPES)
def test_k13h_is_deterministic_and_graph_safe(dtype, hip_lib):
    from metrabs_amd import kernels
    for shape in [(64, 960, 160, 16, 16), (64, 160, 960, 16, 16), (64, 1536, 256, 8, 8)]:
        x, w, b, gt, r = _inputs(*shape, 3, True, True, dtype)
        a = kernels.conv1x1_bias_act16(x, w, b, 'silu', gate=gt, residual=r)
        assert torch.equal(a, kernels.conv1x1_bias_act16(x, w, b, 'silu', gate=gt, residual=r))
        with torch.inference_mode():
            out = torch.empty_like(a)
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                kernels.conv1x1_bias_act16(x, w, b, 'silu', gate=gt, residual=r, out=out)
                st.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                    kernels.conv1x1_bias_act16(x, w, b, 'silu', gate=gt, residual=r, out=out)
            torch.cuda.current_stream().wait_stream(st)
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, a)


def test_k13h_entry_point_argument_checks(hip_lib):
    """No GPU work: every call below is refused before a launch (the output stays untouched)."""
    null = ctypes.c_void_p(0)
    t = torch.zeros(1024, device='cuda', dtype=torch.float16)
    sentinel = torch.full((512,), 7.0, device='cuda', dtype=torch.float16)
    p = ctypes.c_void_p(t.data_ptr())
    q = ctypes.c_void_p(sentinel.data_ptr())
    f = hip_lib.mtr_conv1x1_bias_act16
    assert f(null, 1, p, p, null, null, 0, 1, 8, 8, 16, q, null) == -1     # MTR_E_NULL
    assert f(p, 1, null, p, null, null, 0, 1, 8, 8, 16, q, null) == -1
    assert f(p, 1, p, null, null, null, 0, 1, 8, 8, 16, q, null) == -1
    assert f(p, 1, p, p, null, null, 0, 1, 8, 8, 16, null, null) == -1
    assert f(p, 0, p, p, null, null, 0, 1, 8, 8, 16, q, null) == -3        # f32: K13's entry
    assert f(p, 3, p, p, null, null, 0, 1, 8, 8, 16, q, null) == -3
    assert f(p, 1, p, p, null, null, 0, 1, 8, 8, 49, q, null) == -2        # H*W = 49
    assert f(p, 1, p, p, null, null, 0, 1, 8, 8, 36, q, null) == -2        # H*W = 36: not a multiple of 8
    assert f(p, 1, p, p, null, null, 0, 1, 8, 12, 16, q, null) == -2       # Cin = 12
    assert f(p, 1, p, p, null, null, 0, 1, 0, 8, 16, q, null) == -2        # Cout = 0
    assert f(p, 1, p, p, null, null, 0, -1, 8, 8, 16, q, null) == -2       # B < 0
    assert f(p, 1, p, p, null, null, 7, 1, 8, 8, 16, q, null) == -4        # act code
    assert f(p, 2, p, p, null, null, 0, 1, 8, 8, 16, p, null) == -4        # y aliases x
    assert f(p, 2, p, p, null, p, 0, 1, 8, 8, 16, q, null) == -4           # residual aliases x
    odd = ctypes.c_void_p(t.data_ptr() + 8)
    assert f(odd, 1, p, p, null, null, 0, 1, 8, 8, 16, q, null) == -6      # misaligned x, weight, y, residual
    assert f(p, 1, odd, p, null, null, 0, 1, 8, 8, 16, q, null) == -6
    assert f(p, 1, p, p, null, null, 0, 1, 8, 8, 16, odd, null) == -6
    assert f(p, 1, p, p, null, odd, 0, 1, 8, 8, 16, q, null) == -6
    assert f(p, 1, p, p, null, null, 0, 0, 8, 8, 16, q, null) == 0         # B = 0: nothing to do
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())


def _calibrated(name, res, batch_size=4):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    return backbones.calibrate_batchnorm(backbones.build_backbone(name).cuda(), res, 'cuda', batch_size=batch_size)


def _eligible_1x1(m, x_shape):
    c = m.conv
    return (c.kernel_size == (1, 1) and c.stride == (1, 1) and not m.emit_mean and c.in_channels % 8 == 0
            and (x_shape[2] * x_shape[3]) % 8 == 0)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('res', [256, 224, 160])
@pytest.mark.parametrize('name', ['efficientnetv2-s', 'efficientnetv2-l', 'mobilenetv3', 'resnet18'])
def test_copy_on_every_backbone(name, res, dtype, hip_lib):
    """The 16-bit copy runs (NCHW and channels_last input), holds the documented parameter dtypes, takes K13h on
    every eligible 1x1 layer, and is as close to the f32 network as the f32 copy under autocast of its dtype."""
    from metrabs_amd import backbones
    net = _calibrated(name, res)
    f32 = backbones.fold_batchnorm(net, fused_epilogue=True)
    c16 = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype)
    assert c16.inference_dtype == dtype and getattr(f32, 'inference_dtype', None) is None
    for m in c16.modules():
        if isinstance(m, backbones.ConvBiasAct):
            assert m.conv.weight.dtype == dtype and m.bias.dtype == torch.float32
        elif isinstance(m, backbones.DepthwiseBiasAct):
            assert m.weight.dtype == torch.float32 and m.bias.dtype == torch.float32
        elif isinstance(m, backbones.SqueezeExcite):
            assert all(p.dtype == torch.float32 for p in m.parameters())
    x = torch.rand(8, 3, res, res, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    seen = {}

    def hook(mod, args, kwargs):
        seen[mod] = tuple(args[0].shape)

    hs = [m.register_forward_pre_hook(hook, with_kwargs=True) for m in c16.modules()
          if isinstance(m, backbones.ConvBiasAct)]
    with torch.inference_mode():
        a = f32(x)
        with torch.autocast('cuda', dtype=dtype):
            b = f32(x)
        c = c16(x)
        for h in hs:
            h.remove()
        paths = {m: m.last_path for m in seen}
        # channels_last input (what Metrabs.predict_multi hands the backbone): the library path everywhere
        x_cl = x.to(memory_format=torch.channels_last)
        d = c16(x_cl)
        with torch.autocast('cuda', dtype=dtype):
            b_cl = f32(x_cl)
    assert c.dtype == dtype and b.dtype == dtype and d.dtype == dtype and c.shape == a.shape
    for m, p in paths.items():
        if _eligible_1x1(m, seen[m]) and (m.conv.in_channels, m.conv.out_channels,
                                          seen[m][2] * seen[m][3]) not in backbones.ConvBiasAct.k13h_slower:
            assert p in ('k13h', 'k13h_gate'), (m, seen[m], p)
        else:
            assert p == 'library', (m, seen[m], p)
    if res == 256 and name != 'resnet18':   # (at 224 px the gated 14x14 / 7x7 projects are not eligible)
        assert 'k13h_gate' in paths.values()
    a = a.float()
    mean_c, mean_b = float((c.float() - a).abs().mean()), float((b.float() - a).abs().mean())
    amax = float(a.abs().max())
    assert mean_c <= 1.1 * mean_b + 1e-6 * amax, (mean_c, mean_b)
    # max-abs: test_gpu_bias_act's autocast bound, 0.1 max|f32|, wherever autocast of the same dtype meets it itself.
    # It does not for EfficientNetV2-L at 256 / 224 / 160 px in f16 and bf16, nor for EfficientNetV2-S and
    # MobileNetV3 in bf16 at all three sizes (autocast 0.23 - 0.76 max|f32| there, profiles/r09a_copy_accuracy.jsonl):
    # there the copy may not be worse than autocast by more than 10 %
    max_c, max_b = float((c.float() - a).abs().max()), float((b.float() - a).abs().max())
    if max_b <= 0.1 * amax:
        assert max_c <= 0.1 * amax, (max_c, max_b, amax)
    else:
        assert max_c <= 1.1 * max_b, (max_c, max_b, amax)
    assert torch.isfinite(d).all()
    mean_d, mean_b_cl = float((d.float() - a).abs().mean()), float((b_cl.float() - a).abs().mean())
    assert mean_d <= 1.1 * mean_b_cl + 1e-6 * amax, (mean_d, mean_b_cl)


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


def _poses(est, images, boxes):
    with torch.inference_mode():
        r = est.estimate_poses_batched(images, boxes, num_aug=2)
    return torch.cat(r['poses3d']).clone()


def test_copy_through_the_loader_and_the_api(tmp_path, hip_lib):
    from metrabs_amd import backbones, loading
    d = _model_dir(tmp_path)
    ref = loading.load_multiperson_model(d)
    auto = loading.load_multiperson_model(d)
    auto.crop_model.autocast_dtype = torch.float16    # the reference's GPU arithmetic (bench.py's f16 mode)
    auto.crop_model.deterministic_backbone = True
    auto.crop_dtype = torch.float16
    est = loading.load_multiperson_model(d, dtype=torch.float16)
    assert ref.crop_dtype == torch.float32 and ref.crop_model.input_dtype == torch.float32
    assert est.crop_dtype == torch.float16 and est.crop_model.input_dtype == torch.float16
    assert est.crop_model.backbone.inference_dtype == torch.float16
    assert ref.crop_model.backbone_is_pinned() and not est.crop_model.backbone_is_pinned()
    assert loading.load_crop_model(d, dtype=torch.bfloat16).input_dtype == torch.bfloat16
    assert loading.load_crop_model(d, dtype=torch.float32).input_dtype == torch.float32
    # MPJPE to the f32 model, summed over three calls (per call the two are 0.1 - 0.5 mm apart on this synthetic
    # model, and either can be the smaller one): no absolute slack
    e16 = e_auto = 0.0
    for seed in (5, 9, 13):
        images, boxes = _api_inputs(seed)
        p_ref, p_auto, p16 = _poses(ref, images, boxes), _poses(auto, images, boxes), _poses(est, images, boxes)
        assert torch.isfinite(p16).all() and p16.shape == p_ref.shape
        e16 += float((p16 - p_ref).norm(dim=-1).mean())
        e_auto += float((p_auto - p_ref).norm(dim=-1).mean())
    paths = [m.last_path for m in est.crop_model.backbone.modules() if isinstance(m, backbones.ConvBiasAct)]
    assert 'k13h' in paths and 'k13h_gate' in paths
    assert 0 < e16 <= 1.1 * e_auto, (e16, e_auto)

    # pinned: a graphed call returns the eager call's bits
    est.crop_model.deterministic_backbone = True
    eager = loading.load_multiperson_model(d, dtype=torch.float16)
    eager.crop_model.deterministic_backbone = True
    eager.graph_batches = False
    est.graph_batches = True
    for seed in (5, 9):
        images, boxes = _api_inputs(seed)
        a, b = _poses(eager, images, boxes), _poses(est, images, boxes)
        assert torch.equal(a, b), float((a - b).abs().max())
    assert est.graphs.stats['captures'] >= 1 and est.graphs.stats['replays'] >= 1, est.graphs.stats

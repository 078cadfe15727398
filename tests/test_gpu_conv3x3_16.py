"""GPU: K14h (csrc/conv3x3_16.hip), the dense 3x3 convolution of the 16-bit inference copy as one implicit 16-bit
MFMA GEMM with the K10 epilogue: against fp64 on every dense 3x3 shape of the EfficientNetV2 backbones, every
epilogue and edge geometry, determinism and graph replay, argument checks; the Conv3x3BiasAct module in the copy of
every backbone (paths, fallbacks, the untouched f32 copy, accuracy against the library path); through the API."""
import ctypes
import functools

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
BACKBONES = ['efficientnetv2-s', 'efficientnetv2-l', 'mobilenetv3', 'resnet18']


@functools.lru_cache(maxsize=None)
def _conv3x3_shapes(name, res):
    """(Cin, Cout, H, W, stride, act, residual) of every Conv3x3BiasAct of a 16-bit copy at `res` px."""
    from metrabs_amd import backbones
    net = backbones.fold_batchnorm(backbones.build_backbone(name).eval(), fused_epilogue=True,
                                   dtype=torch.float16).cuda()
    shapes = set()

    def hook(mod, args, kwargs):
        x = args[0]
        shapes.add((x.shape[1], mod.conv.out_channels, x.shape[2], x.shape[3], mod.stride, mod.act_name,
                    kwargs.get('residual') is not None))

    hs = [m.register_forward_pre_hook(hook, with_kwargs=True) for m in net.modules()
          if isinstance(m, backbones.Conv3x3BiasAct)]
    assert hs
    backbones.Conv3x3BiasAct.use_k14h = False
    try:
        with torch.inference_mode():
            net(torch.rand(1, 3, res, res, device='cuda'))
    finally:
        backbones.Conv3x3BiasAct.use_k14h = True
    for h in hs:
        h.remove()
    return tuple(sorted(shapes, key=str))


def _inputs(B, K, M, H, W, stride, seed, residual, dtype, border=1.0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(B, K, H, W, device='cuda', generator=g)
    if border != 1.0:   # large border pixels: a wrong halo (a missed or a doubled edge tap) shows
        edge = torch.ones(H, W, device='cuda')
        edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = border
        x = x * edge
    x = x.to(dtype)
    w = (torch.randn(M, K, 3, 3, device='cuda', generator=g) / (9 * K) ** 0.5).to(dtype)
    b = 0.5 * torch.randn(M, device='cuda', generator=g)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    r = torch.randn(B, M, Ho, Wo, device='cuda', generator=g).to(dtype) if residual else None
    return x, w, b, r


def _reference(x, w, b, act, stride, r):
    """(fp64 result, bound).  test_gpu_backbone16._check with K = 9 Cin: |got - fp64| <= one unit in the last place of
    the 16-bit result + 1.1 K 2^-24 sum |w| |x| (f32 accumulation through the activation, Lipschitz <= 1.1) +
    1e-6 |ref| + 2^-24.  The fp64 reference is F.conv2d on the 16-bit operands cast to double."""
    dt = x.dtype
    K = 9 * x.shape[1]
    z = F.conv2d(x.double(), w.double(), None, stride, 1) + b.double()[None, :, None, None]
    s = F.conv2d(x.double().abs(), w.double().abs(), None, stride, 1) + b.double().abs()[None, :, None, None]
    ref = _TORCH_ACT[act](z)
    if r is not None:
        ref = ref + r.double()
    tiny = torch.finfo(dt).tiny
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(tiny))) - _MANT[dt])
    return ref, ulp + 1.1 * K * 2.0 ** -24 * s + 1e-6 * ref.abs() + 2.0 ** -24


def _check(x, w, b, act, stride, r, got):
    """_reference's bound on every element (tests/conv_fuzz.py uses the same two functions)."""
    dt = x.dtype
    ref, bound = _reference(x, w, b, act, stride, r)
    assert got.shape == ref.shape and got.dtype == dt
    err = (got.double() - ref).abs()
    print(f'k14h check {tuple(x.shape)} -> {tuple(got.shape)} s{stride} {act} {dt}: '
          f'max err / bound = {float((err / bound).max()):.3f}')
    excess = float((err - bound).max())
    assert excess <= 0, excess


_BENCH_BATCH = {'efficientnetv2-s': 64, 'efficientnetv2-l': 32}


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name,res', [('efficientnetv2-s', 256), ('efficientnetv2-s', 224), ('efficientnetv2-s', 160),
                                      ('efficientnetv2-l', 384)])
@pytest.mark.parametrize('B', [1, 3, 'bench'])
def test_k14h_matches_fp64_on_every_dense_3x3_shape(name, res, B, dtype, hip_lib):
    from metrabs_amd import kernels
    shapes = _conv3x3_shapes(name, res)
    assert len(shapes) >= 5
    ran = 0
    for i, (K, M, H, W, stride, act, res_) in enumerate(shapes):
        n = _BENCH_BATCH[name] if B == 'bench' else B
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        if B == 'bench' and n * M * Ho * Wo > 2 ** 26:
            continue   # (the fp64 reference of the largest maps at the bench batch: covered at B = 1, 3)
        x, w, b, r = _inputs(n, K, M, H, W, stride, 2000 + i, res_, dtype)
        wp = kernels.pack_conv3x3_weight(w)
        assert kernels.conv3x3_16_supported(x, wp, stride), (K, M, H, W, stride)
        _check(x, w, b, act, stride, r, kernels.conv3x3_bias_act16(x, wp, b, act, stride, residual=r))
        ran += 1
    assert ran >= 3


# (Cin, Cout, H, W): maps that are not a multiple of the tile, a non-square one, Cout not a multiple of 32
EDGE_SHAPES = [(8, 24, 20, 20), (24, 72, 28, 28), (40, 24, 12, 12), (96, 72, 8, 8), (24, 96, 12, 20), (40, 160, 20, 12)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('residual', [False, True])
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('shape', EDGE_SHAPES)
def test_k14h_every_epilogue_and_edge_geometry(act, residual, stride, shape, dtype, hip_lib):
    from metrabs_amd import kernels
    K, M, H, W = shape
    if stride == 2:
        H, W = 2 * H, 2 * W   # the same output maps behind a stride-2 layer
    x, w, b, r = _inputs(3, K, M, H, W, stride, 7, residual, dtype, border=8.0)
    wp = kernels.pack_conv3x3_weight(w)
    assert kernels.conv3x3_16_supported(x, wp, stride)
    _check(x, w, b, act, stride, r, kernels.conv3x3_bias_act16(x, wp, b, act, stride, residual=r))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('shape', [(24, 40, 12, 24), (16, 200, 36, 8)])
def test_k14h_is_exact_on_small_integers(shape, stride, dtype, hip_lib):
    """Small-integer data with an asymmetric weight (every tap and input channel distinct, no symmetry in ky, kx or
    ci): every product and partial sum is an integer below 2^8 (bf16's exact range), so the result must be exact --
    a swapped tap, a transposed fragment or a wrong halo cannot hide in rounding."""
    from metrabs_amd import kernels
    K, M, H, W = shape
    g = torch.Generator(device='cuda').manual_seed(3)
    x = torch.randint(-2, 3, (2, K, H, W), device='cuda', generator=g).float()
    w = torch.zeros(M, K, 3, 3, device='cuda')
    m = torch.arange(M, device='cuda')
    for t in range(9):   # output channel m looks at tap t of input channel (m + 5 t) % K only, weight -(t + 1) or t + 1
        w[m, (m + 5 * t) % K, t // 3, t % 3] = torch.where(m % 2 == 0, t + 1.0, -(t + 1.0))
    b = torch.arange(M, device='cuda').float() % 7 - 3
    ref = F.conv2d(x.double(), w.double(), b.double(), stride, 1)
    assert float(ref.abs().max()) <= 2 * 45 + 3 < 2 ** 8
    got = kernels.conv3x3_bias_act16(x.to(dtype), kernels.pack_conv3x3_weight(w.to(dtype)), b, None, stride)
    assert torch.equal(got.double(), ref)


@pytest.mark.parametrize('dtype', DTYPES)
def test_k14h_is_deterministic_and_graph_safe(dtype, hip_lib):
    from metrabs_amd import kernels
    for (B, K, M, H, W, stride, res_) in [(8, 24, 24, 128, 128, 1, True), (8, 48, 192, 64, 64, 1, False),
                                          (8, 64, 256, 64, 64, 2, False), (3, 40, 72, 20, 12, 1, True)]:
        x, w, b, r = _inputs(B, K, M, H, W, stride, 3, res_, dtype)
        wp = kernels.pack_conv3x3_weight(w)
        a = kernels.conv3x3_bias_act16(x, wp, b, 'silu', stride, residual=r)
        assert torch.equal(a, kernels.conv3x3_bias_act16(x, wp, b, 'silu', stride, residual=r))
        with torch.inference_mode():
            out = torch.empty_like(a)
            assert kernels.conv3x3_bias_act16(x, wp, b, 'silu', stride, residual=r, out=out) is out
            assert torch.equal(out, a)   # an out= call equals the allocating call
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                kernels.conv3x3_bias_act16(x, wp, b, 'silu', stride, residual=r, out=out)
                st.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                    kernels.conv3x3_bias_act16(x, wp, b, 'silu', stride, residual=r, out=out)
            torch.cuda.current_stream().wait_stream(st)
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, a)


def test_k14h_entry_point_argument_checks(hip_lib):
    """No GPU work: every call below is refused before a launch (the output stays untouched)."""
    from metrabs_amd import kernels
    null = ctypes.c_void_p(0)
    t = torch.zeros(8192, device='cuda', dtype=torch.float16)
    sentinel = torch.full((4096,), 7.0, device='cuda', dtype=torch.float16)
    p = ctypes.c_void_p(t.data_ptr())
    q = ctypes.c_void_p(sentinel.data_ptr())
    f = hip_lib.mtr_conv3x3_bias_act16
    # f(x, dtype, weight, bias, residual, act, B, Cin, Cout, H, W, stride, y, stream)
    assert f(null, 1, p, p, null, 0, 1, 8, 8, 8, 8, 1, q, null) == -1      # MTR_E_NULL
    assert f(p, 1, null, p, null, 0, 1, 8, 8, 8, 8, 1, q, null) == -1
    assert f(p, 1, p, null, null, 0, 1, 8, 8, 8, 8, 1, q, null) == -1
    assert f(p, 1, p, p, null, 0, 1, 8, 8, 8, 8, 1, null, null) == -1
    assert f(p, 0, p, p, null, 0, 1, 8, 8, 8, 8, 1, q, null) == -3         # f32
    assert f(p, 3, p, p, null, 0, 1, 8, 8, 8, 8, 1, q, null) == -3
    assert f(p, 1, p, p, null, 0, 1, 12, 8, 8, 8, 1, q, null) == -2        # Cin = 12
    assert f(p, 1, p, p, null, 0, 1, 3, 8, 8, 8, 1, q, null) == -2         # Cin = 3 (the stem)
    assert f(p, 1, p, p, null, 0, 1, 8, 8, 8, 8, 3, q, null) == -2         # stride 3
    assert f(p, 1, p, p, null, 0, 1, 8, 8, 8, 8, 0, q, null) == -2
    assert f(p, 1, p, p, null, 0, 1, 8, 8, 8, 7, 1, q, null) == -2         # W = 7
    assert f(p, 1, p, p, null, 0, 1, 8, 8, 8, 12, 2, q, null) == -2        # W = 12, stride 2: Wo = 6
    assert f(p, 1, p, p, null, 0, 1, 8, 0, 8, 8, 1, q, null) == -2         # Cout = 0
    assert f(p, 1, p, p, null, 0, -1, 8, 8, 8, 8, 1, q, null) == -2        # B < 0
    assert f(p, 1, p, p, null, 0, 1, 512, 8, 8, 8, 1, q, null) == -2       # the halo of 512 channels: not in LDS
    assert f(p, 1, p, p, null, 7, 1, 8, 8, 8, 8, 1, q, null) == -4         # act code
    assert f(p, 2, p, p, null, 0, 1, 8, 8, 8, 8, 1, p, null) == -4         # y aliases x
    assert f(p, 2, p, p, q, 0, 1, 8, 8, 8, 8, 1, q, null) == -4            # y aliases the residual
    odd = ctypes.c_void_p(t.data_ptr() + 8)
    assert f(odd, 1, p, p, null, 0, 1, 8, 8, 8, 8, 1, q, null) == -6       # misaligned x, weight, y, residual
    assert f(p, 1, odd, p, null, 0, 1, 8, 8, 8, 8, 1, q, null) == -6
    assert f(p, 1, p, p, null, 0, 1, 8, 8, 8, 8, 1, odd, null) == -6
    assert f(p, 1, p, p, odd, 0, 1, 8, 8, 8, 8, 1, q, null) == -6
    assert f(p, 1, p, p, null, 0, 0, 8, 8, 8, 8, 1, q, null) == 0          # B = 0: nothing to do
    assert hip_lib.mtr_conv3x3_16_lds_bytes(1, 8, 8, 8, 8, 1) > 0
    assert hip_lib.mtr_conv3x3_16_lds_bytes(1, 8, 8, 8, 8, 3) == 0
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())

    # the wrapper: an OIHW weight (right element count, wrong layout), a wrong element count, a residual of the wrong
    # shape or dtype, a misaligned x
    x, w, b, r = _inputs(2, 8, 16, 8, 8, 1, 1, True, torch.float16)
    wp = kernels.pack_conv3x3_weight(w)
    with pytest.raises(ValueError):
        kernels.conv3x3_bias_act16(x, w, b, None, 1)
    with pytest.raises(ValueError):
        kernels.conv3x3_bias_act16(x, wp[:, :, :, :4].contiguous(), b, None, 1)
    with pytest.raises(ValueError):
        kernels.conv3x3_bias_act16(x, wp, b, None, 1, residual=r[:, :, :4].contiguous())
    with pytest.raises(ValueError):
        kernels.conv3x3_bias_act16(x, wp, b, None, 1, residual=r.bfloat16())
    with pytest.raises(ValueError):
        kernels.conv3x3_bias_act16(x, wp, b, None, 3)
    with pytest.raises(ValueError):
        kernels.conv3x3_bias_act16(x, wp.bfloat16(), b, None, 1)
    flat = torch.zeros(x.numel() + 4, device='cuda', dtype=torch.float16)
    x_off = flat[4:].view_as(x)   # 8 bytes past a 16-byte boundary
    assert not kernels.conv3x3_16_supported(x_off, wp, 1)
    with pytest.raises(RuntimeError):
        kernels.conv3x3_bias_act16(x_off, wp, b, None, 1)
    assert not kernels.conv3x3_16_supported(x, wp, 3)
    assert not kernels.conv3x3_16_supported(x.to(memory_format=torch.channels_last), wp, 1)
    assert not kernels.conv3x3_16_supported(x.float(), wp, 1)
    assert kernels.conv3x3_16_supported(x, wp, 1)


def _calibrated(name, res, batch_size=4):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    return backbones.calibrate_batchnorm(backbones.build_backbone(name).cuda(), res, 'cuda', batch_size=batch_size)


def _module_paths(net, cls):
    return [(type(m).__name__, getattr(m, 'last_path', None)) for m in net.modules() if isinstance(m, cls)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', BACKBONES)
def test_copy_takes_k14h_where_it_applies(name, dtype, hip_lib):
    from metrabs_amd import backbones, kernels
    C3 = backbones.Conv3x3BiasAct
    assert not issubclass(C3, backbones.ConvBiasAct)
    res = 256
    net = _calibrated(name, res)
    f32 = backbones.fold_batchnorm(net, fused_epilogue=True)
    c16 = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype)
    mods = [m for m in c16.modules() if isinstance(m, C3)]
    if name == 'mobilenetv3':
        assert not mods   # (no dense 3x3 layer with Cin % 8 == 0)
    else:
        assert mods
    for m in mods:
        assert m.conv.weight.dtype == dtype and m.weight_packed.dtype == dtype and m.bias.dtype == torch.float32
        assert torch.equal(m.weight_packed, m.conv.weight.permute(0, 2, 3, 1))
    x = torch.rand(8, 3, res, res, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    seen = {}

    def hook(mod, args, kwargs):
        seen[mod] = args[0]

    hs = [m.register_forward_pre_hook(hook, with_kwargs=True) for m in mods]
    try:
        with torch.inference_mode():
            a = f32(x).float()
            on = c16(x)
            for m in mods:
                xin = seen[m]
                key = (m.conv.in_channels, m.conv.out_channels, m.stride, xin.shape[2], xin.shape[3])
                want = kernels.conv3x3_16_supported(xin.to(dtype).contiguous(), m.weight_packed, m.stride) \
                    and key not in C3.k14h_slower
                assert m.last_path == ('k14h' if want else 'library'), (key, m.last_path)
            if name.startswith('efficientnet'):
                assert sum(m.last_path == 'k14h' for m in mods) >= 1 or all(
                    (m.conv.in_channels, m.conv.out_channels, m.stride, seen[m].shape[2], seen[m].shape[3])
                    in C3.k14h_slower for m in mods)
            # channels_last input: the library path everywhere
            c16(x.to(memory_format=torch.channels_last))
            assert all(m.last_path == 'library' for m in mods)
            C3.use_k14h = False
            off = c16(x)
            assert all(m.last_path == 'library' for m in mods)
            C3.use_k14h = True
    finally:
        C3.use_k14h = True
        for h in hs:
            h.remove()
    assert on.dtype == dtype and torch.isfinite(on).all()
    # no further from the f32 network than the library path (test_copy_on_every_backbone's criterion and margin)
    mean_on, mean_off = float((on.float() - a).abs().mean()), float((off.float() - a).abs().mean())
    print(f'{name} {dtype}: mean |copy - f32| k14h on {mean_on:.6g} off {mean_off:.6g} max|f32| {float(a.abs().max()):.4g}')
    assert mean_on <= 1.1 * mean_off + 1e-6 * float(a.abs().max()), (mean_on, mean_off)


@pytest.mark.parametrize('name', BACKBONES)
def test_f32_copy_is_untouched(name, hip_lib):
    """fold_batchnorm(dtype=None): no Conv3x3BiasAct, the same module types and paths and -- under the deterministic
    pin the f32 model runs with -- the same bits whether the K14h switch is on or off."""
    from metrabs_amd import backbones
    C3 = backbones.Conv3x3BiasAct
    net = _calibrated(name, 256)
    f32 = backbones.fold_batchnorm(net, fused_epilogue=True)
    assert not any(isinstance(m, C3) for m in f32.modules())
    x = torch.rand(4, 3, 256, 256, device='cuda', generator=torch.Generator(device='cuda').manual_seed(2))
    outs, trees = [], []
    try:
        for sw in (True, False):
            C3.use_k14h = sw
            with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
                outs.append(f32(x).clone())
            trees.append([(type(m).__name__, getattr(m, 'last_path', None)) for m in f32.modules()])
    finally:
        C3.use_k14h = True
    assert trees[0] == trees[1]
    assert torch.equal(outs[0], outs[1])


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


def test_k14h_through_the_loader_and_the_api(tmp_path, hip_lib):
    from metrabs_amd import backbones, loading
    d = _model_dir(tmp_path)
    est = loading.load_multiperson_model(d, dtype=torch.float16)
    est.crop_model.deterministic_backbone = True
    est.graph_batches = True
    eager = loading.load_multiperson_model(d, dtype=torch.float16)
    eager.crop_model.deterministic_backbone = True
    eager.graph_batches = False
    for seed in (5, 9):
        images, boxes = _api_inputs(seed)
        a, b = _poses(eager, images, boxes), _poses(est, images, boxes)
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), float((a - b).abs().max())   # a graphed call returns the eager call's bits
    for model in (est, eager):
        paths = [m.last_path for m in model.crop_model.backbone.modules()
                 if isinstance(m, backbones.Conv3x3BiasAct)]
        assert 'k14h' in paths, paths
    assert est.graphs.stats['captures'] >= 1 and est.graphs.stats['replays'] >= 1, est.graphs.stats

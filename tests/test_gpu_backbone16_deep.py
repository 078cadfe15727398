"""GPU: fold_batchnorm(dtype=, deep_projects=True) -- the deep project convolutions of the 16-bit copy on K13h's deep-K
configuration: which path every armed layer takes, that no x * gate pass runs in front of one, the bits of the same
copy on K13h's old tiles, the accuracy criteria of the default copy (tests/test_gpu_backbone16.py), every fall-back,
and the option through the loader and the drop-in API."""
import functools

import numpy as np
import pytest
import torch
from torch.overrides import TorchFunctionMode

from oracle import cases

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = [F16, BF16]
DEEP = ('k13h_deep', 'k13h_deep_gate')


@functools.lru_cache(maxsize=None)
def _calibrated(name, res):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    return backbones.calibrate_batchnorm(backbones.build_backbone(name).cuda(), res, 'cuda', batch_size=4)


def _armed_layers(net):
    from metrabs_amd import backbones
    return [m for m in net.modules() if isinstance(m, backbones.ConvBiasAct) and m.deep_projects]


class _CountWideMultiplies(TorchFunctionMode):
    """Records the shape of every torch multiply whose first operand is a 4-D tensor of at least 768 channels: the
    `x * gate` pass of a squeeze-excite block in front of a deep project (nothing else in these networks multiplies
    such a tensor)."""

    def __init__(self):
        super().__init__()
        self.shapes = []

    def __torch_function__(self, func, types, args=(), kwargs=None):
        if func in (torch.Tensor.mul, torch.Tensor.__mul__, torch.mul, torch.Tensor.mul_) and args \
                and isinstance(args[0], torch.Tensor) and args[0].dim() == 4 and args[0].shape[1] >= 768:
            self.shapes.append(tuple(args[0].shape))
        return func(*args, **(kwargs or {}))


def _pinned():
    """The library convolutions under the deterministic pin (Metrabs.deterministic_backbone): without it MIOpen may
    answer the first call of a shape with another solution than the later ones, and two library paths are compared
    bit for bit here."""
    return torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True)


def _run(net, x):
    """-> (features, {armed layer: (input shape, last_path)}, shapes of the wide multiplies)."""
    seen = {}
    hs = [m.register_forward_pre_hook(lambda mod, args, kwargs: seen.__setitem__(mod, tuple(args[0].shape)),
                                      with_kwargs=True) for m in _armed_layers(net)]
    try:
        with torch.inference_mode(), _pinned(), _CountWideMultiplies() as counter:
            y = net(x)
    finally:
        for h in hs:
            h.remove()
    return y, {m: (seen[m], m.last_path) for m in seen}, counter.shapes


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name,n_armed', [('efficientnetv2-s', 15), ('efficientnetv2-l', 60)])
def test_armed_copy_runs_its_deep_projects_on_the_deep_config(name, n_armed, dtype, hip_lib):
    """256 px, batch 2: the armed maps are 16x16 and 8x8, and every armed layer stands behind a squeeze-excite block
    that hands its gate over."""
    from metrabs_amd import backbones
    C = backbones.ConvBiasAct
    net = _calibrated(name, 256)
    f32 = backbones.fold_batchnorm(net, fused_epilogue=True)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, deep_projects=True)
    assert list(plain.state_dict()) == list(armed.state_dict())
    assert len(_armed_layers(armed)) == n_armed and not _armed_layers(plain)
    x = torch.rand(2, 3, 256, 256, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    c, paths, muls = _run(armed, x)
    assert len(paths) == n_armed
    for m, (shape, path) in paths.items():
        assert path in DEEP, (m, shape, path)
        assert shape[2] * shape[3] in (256, 64)
    assert 'k13h_deep_gate' in {p for _, p in paths.values()}
    assert muls == []                       # no x * gate pass in front of an armed layer
    _, _, muls_plain = _run_plain(plain, x)
    # ... which the default copy runs for its listed-slower projects: 14 x 1536 -> 256 at 8x8 of EfficientNetV2-S
    # (EfficientNetV2-L's listed shapes are those of 384 px: at 256 px its default copy runs K13h with the gate)
    assert len(muls_plain) == (14 if name == 'efficientnetv2-s' else 0)
    # the same layers on K13h's old tiles: the same bits
    try:
        C.deep_config = 'auto'
        c_auto, paths_auto, muls_auto = _run(armed, x)
    finally:
        C.deep_config = 'deepk'
    assert torch.equal(c, c_auto) and muls_auto == []
    assert {m: p for m, (_, p) in paths_auto.items()} == {m: p for m, (_, p) in paths.items()}
    # the accuracy criteria of the default copy: mean-abs and max-abs against the f32 folded network, relative to
    # the f32 copy under autocast of the same dtype
    with torch.inference_mode(), _pinned():
        a = f32(x)
        with torch.autocast('cuda', dtype=dtype):
            b = f32(x)
    assert c.dtype == dtype and c.shape == a.shape and torch.isfinite(c).all()
    a = a.float()
    mean_c, mean_b = float((c.float() - a).abs().mean()), float((b.float() - a).abs().mean())
    amax = float(a.abs().max())
    assert mean_c <= 1.1 * mean_b + 1e-6 * amax, (mean_c, mean_b)
    max_c, max_b = float((c.float() - a).abs().max()), float((b.float() - a).abs().max())
    if max_b <= 0.1 * amax:
        assert max_c <= 0.1 * amax, (max_c, max_b, amax)
    else:
        assert max_c <= 1.1 * max_b, (max_c, max_b, amax)


def _run_plain(net, x):
    with torch.inference_mode(), _pinned(), _CountWideMultiplies() as counter:
        y = net(x)
    return y, None, counter.shapes


@pytest.mark.parametrize('dtype', DTYPES)
def test_6x6_maps_fall_back_with_the_default_copys_bits(dtype, hip_lib):
    """EfficientNetV2-L at 192 px: the 12x12 projects run K13h either way (every configuration returns the same bits),
    the 6x6 ones (36 positions: no 16-byte groups) take the library path as in the default copy."""
    from metrabs_amd import backbones
    net = _calibrated('efficientnetv2-l', 192)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, deep_projects=True)
    x = torch.rand(1, 3, 192, 192, device='cuda', generator=torch.Generator(device='cuda').manual_seed(2))
    with torch.inference_mode(), _pinned():
        want = plain(x)
    got, paths, _ = _run(armed, x)
    assert len(paths) == 60
    for m, (shape, path) in paths.items():
        assert path == ('library' if shape[2] * shape[3] == 36 else 'k13h_deep_gate'), (shape, path)
    assert {s[2] * s[3] for s, _ in paths.values()} == {144, 36}
    assert torch.equal(got, want)


@pytest.mark.parametrize('dtype', DTYPES)
def test_an_armed_layer_keeps_todays_branch_where_it_must(dtype, hip_lib):
    from metrabs_amd import backbones
    C = backbones.ConvBiasAct
    net = _calibrated('efficientnetv2-s', 256)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, deep_projects=True)
    pairs = [(a, p) for a, p in zip(armed.modules(), plain.modules())
             if isinstance(a, C) and a.deep_projects and a.conv.in_channels == 1536]
    assert len(pairs) == 14
    a, p = pairs[0]
    g = torch.Generator(device='cuda').manual_seed(3)
    x = torch.randn(2, 1536, 8, 8, device='cuda', generator=g).to(dtype)
    r = torch.randn(2, 256, 8, 8, device='cuda', generator=g).to(dtype)
    assert (1536, 256, 64) in C.k13h_slower
    with torch.inference_mode(), _pinned():
        assert not p.k13h_takes(x) and not a.k13h_takes(x) and a.k13h_deep_takes(x) and not p.k13h_deep_takes(x)
        deep = a(x, residual=r)
        assert a.last_path == 'k13h_deep'                       # called alone: no gate was handed over
        lib = p(x, residual=r)
        assert p.last_path == 'library'
        # K13h against rocBLAS + K10: another summation order, and the library rounds twice (the GEMM's output, then
        # K10's): a few units in the last place of bf16 (2^-8 relative) on values of order 1, no more
        assert torch.allclose(deep.float(), lib.float(), rtol=2.0 ** -6, atol=2.0 ** -6)
        listed = C.k13h_deep_slower
        try:   # a listed shape
            C.k13h_deep_slower = listed | {(1536, 256, 64)}
            assert not a.k13h_deep_takes(x)
            assert torch.equal(a(x, residual=r), lib) and a.last_path == 'library'
        finally:
            C.k13h_deep_slower = listed
        try:   # the class switch of K13h
            C.use_k13h = False
            assert torch.equal(a(x, residual=r), lib) and a.last_path == 'library'
        finally:
            C.use_k13h = True
        with torch.autocast('cuda', dtype=dtype):
            assert torch.equal(a(x, residual=r), p(x, residual=r)) and a.last_path == 'library' == p.last_path
        xt = torch.randn(2, 1536, 8, 16, device='cuda', generator=g).to(dtype)[:, :, :, ::2]   # not contiguous
        assert not xt.is_contiguous()
        assert torch.equal(a(xt), p(xt)) and a.last_path == 'library' == p.last_path
        x6 = torch.randn(2, 1536, 6, 6, device='cuda', generator=g).to(dtype)                   # 36 positions
        assert torch.equal(a(x6), p(x6)) and a.last_path == 'library' == p.last_path
        rs = torch.randn(2, 256, 8, 16, device='cuda', generator=g).to(dtype)[:, :, :, ::2]     # a skip K13h refuses
        assert torch.equal(a(x, residual=rs), p(x, residual=rs)) and a.last_path == 'library'
        assert torch.equal(a(x, residual=r), deep) and a.last_path == 'k13h_deep'
    was = a.conv.weight.requires_grad
    with torch.enable_grad():   # a gradient wanted
        a.conv.weight.requires_grad_(True)
        try:
            assert not a.k13h_deep_takes(x)
        finally:
            a.conv.weight.requires_grad_(was)


# ---- the loader and the API

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


def test_deep_projects_through_the_loader_and_the_api(tmp_path, hip_lib):
    """A 256 px crop model: its 8x8 projects are armed.  Graphed against eager, bit for bit."""
    from metrabs_amd import loading
    d = _model_dir(tmp_path)
    ests = {}
    for key, graphed in [('graph', True), ('eager', False)]:
        est = loading.load_multiperson_model(d, dtype=F16, deep_projects=True)
        est.crop_model.deterministic_backbone = True
        est.graph_batches = graphed
        ests[key] = est
    images = torch.stack([cases.synth_images(1, 240, 320, 5 + i)[0] for i in range(2)]).cuda()
    boxes = [torch.tensor([[60.0, 20.0, 120.0, 200.0], [150.0, 30.0, 100.0, 180.0]]),
             torch.tensor([[40.0, 10.0, 140.0, 210.0]])]
    for _ in range(2):   # (the second call replays the graph)
        a, b = _poses(ests['eager'], images, boxes), _poses(ests['graph'], images, boxes)
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), float((a - b).abs().max())
    for key in ('graph', 'eager'):
        layers = _armed_layers(ests[key].crop_model.backbone)
        assert len(layers) == 15 and {m.last_path for m in layers} == {'k13h_deep_gate'}
    st = ests['graph'].graphs.stats
    assert st['captures'] >= 1 and st['replays'] >= 1, st
    plain = loading.load_crop_model(d, dtype=BF16)
    assert not _armed_layers(plain.backbone)
    assert len(_armed_layers(loading.load_crop_model(d, dtype=BF16, deep_projects=True).backbone)) == 15
    with pytest.raises(ValueError, match='deep_projects'):
        loading.load_crop_model(d, deep_projects=True)

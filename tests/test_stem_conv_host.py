"""CPU: the module side of K17 (backbones.StemConvBiasAct, fold_batchnorm(fuse_stem=True), the loaders): argument
rules, which modules are armed per backbone, unchanged state_dict keys, the library path with the default copy's bits
on CPU tensors, and -- under every fallback condition -- that a tensor Preproc handed over is never convolved without
x * 2 - 1."""
import numpy as np
import pytest
import torch

from oracle import cases

NAMES = ['efficientnetv2-s', 'efficientnetv2-l', 'mobilenetv3']


def _net(name):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    return backbones.build_backbone(name).eval()


def _armed_parts(net):
    from metrabs_amd import backbones
    pre = [m for m in net.modules() if isinstance(m, backbones.Preproc)]
    stems = [m for m in net.modules() if isinstance(m, backbones.StemConvBiasAct)]
    return pre, stems


def test_fold_batchnorm_argument_rules():
    from metrabs_amd import backbones
    net = _net('mobilenetv3')
    with pytest.raises(ValueError, match='fuse_stem'):
        backbones.fold_batchnorm(net, fuse_stem=True)
    with pytest.raises(ValueError, match='fuse_stem'):
        backbones.fold_batchnorm(net, fused_epilogue=False, fuse_stem=True)
    with pytest.raises(ValueError):
        backbones.fold_batchnorm(net, fused_epilogue=True, fuse_stem=True, fuse_blocks=True)   # fuse_blocks: 16 bits
    for dtype in (None, torch.float16, torch.bfloat16):   # independent of dtype and of fuse_blocks
        c = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, fuse_stem=True)
        assert len(_armed_parts(c)[1]) == 1
    c = backbones.fold_batchnorm(_net('efficientnetv2-s'), fused_epilogue=True, dtype=torch.float16, fuse_stem=True,
                                 fuse_blocks=True)
    assert len(_armed_parts(c)[1]) == 1 and any(m.fused_pair for m in c.modules()
                                                if isinstance(m, backbones.FusedMBConv))


@pytest.mark.parametrize('name', NAMES + ['resnet18'])
def test_which_modules_are_armed_and_the_keys_stay(name):
    from metrabs_amd import backbones
    net = _net(name)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, fuse_stem=True)
    assert list(plain.state_dict()) == list(armed.state_dict())
    for (k, a), b in zip(plain.state_dict().items(), armed.state_dict().values()):
        assert torch.equal(a, b), k
    assert backbones.Preproc.hand_to == ()
    assert not _armed_parts(plain)[1] and all('hand_to' not in m.__dict__ for m in _armed_parts(plain)[0])
    pre, stems = _armed_parts(armed)
    if name == 'resnet18':   # a 7x7 stem, no Preproc: nothing to arm
        assert not pre and not stems
        assert [type(m) for m in plain.modules()] == [type(m) for m in armed.modules()]
        return
    assert len(pre) == 1 and len(stems) == 1
    stem = stems[0]
    assert pre[0].hand_to == (stem,) and isinstance(pre[0].hand_to, tuple)
    # the FIRST folded convolution of the network, in the place of the ConvBiasAct of the default copy
    convs = [m for m in armed.modules() if isinstance(m, (backbones.ConvBiasAct, backbones.DepthwiseBiasAct))]
    assert convs[0] is stem and sum(isinstance(m, backbones.StemConvBiasAct) for m in convs) == 1
    c = stem.conv
    assert (c.in_channels, c.kernel_size, c.stride, c.padding, c.bias) == (3, (3, 3), (2, 2), (1, 1), None)
    assert c.out_channels == {'efficientnetv2-s': 24, 'efficientnetv2-l': 32, 'mobilenetv3': 16}[name]
    assert [type(m) for m in plain.modules() if not isinstance(m, backbones.ConvBiasAct)] == \
        [type(m) for m in armed.modules() if not isinstance(m, backbones.ConvBiasAct)]
    assert [n for n, _ in plain.named_modules()] == [n for n, _ in armed.named_modules()]   # nothing registered twice
    assert stem.last_path is None and backbones.StemConvBiasAct.use_k17 is True
    assert isinstance(backbones.StemConvBiasAct.k17_slower, frozenset)


@pytest.mark.parametrize('name', NAMES)
def test_cpu_tensors_take_the_library_path_with_the_default_copys_bits(name):
    from metrabs_amd import backbones
    net = _net(name)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, fuse_stem=True)
    x = torch.rand(2, 3, 64, 64, generator=cases.gen(3))
    with torch.inference_mode():
        a, b = plain(x), armed(x)
        c = armed(x.to(memory_format=torch.channels_last))
        d = plain(x.to(memory_format=torch.channels_last))
    (stem,) = _armed_parts(armed)[1]
    assert stem.last_path == 'library' and stem._handed is None
    assert torch.equal(a, b) and torch.equal(c, d)
    assert [getattr(m, 'last_path', None) for m in plain.modules()] == \
        [getattr(m, 'last_path', None) for m in armed.modules()]


class _Spy(torch.nn.Module):
    """Stands in for the stem's convolution: records what it is asked to convolve."""

    def __init__(self, conv):
        super().__init__()
        self.conv, self.seen = conv, []
        self.weight, self.bias = conv.weight, None
        for k in ('kernel_size', 'stride', 'padding', 'dilation', 'groups', 'padding_mode', 'in_channels',
                  'out_channels'):
            setattr(self, k, getattr(conv, k))

    def forward(self, x):
        self.seen.append(x.clone())
        return self.conv(x)


CONDITIONS = ['cpu', 'switch_off', 'listed', 'gradient', 'autocast', 'odd_shape', 'layout', 'decision_changed']


@pytest.mark.parametrize('cond', CONDITIONS)
def test_a_handed_over_tensor_is_never_convolved_without_preproc(cond, monkeypatch):
    from metrabs_amd import backbones
    S = backbones.StemConvBiasAct
    net = _net('mobilenetv3')
    plain = backbones.fold_batchnorm(net, fused_epilogue=True)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, fuse_stem=True)
    (pre,), (stem,) = _armed_parts(armed)
    plain_stem = next(m for m in plain.modules() if type(m) is backbones.ConvBiasAct and S.applies_to(m.conv))
    spy = stem.conv = _Spy(stem.conv)
    x = torch.rand(2, 3, 32, 32, generator=cases.gen(4))
    grad = torch.enable_grad() if cond == 'gradient' else torch.no_grad()
    if cond == 'switch_off':
        monkeypatch.setattr(S, 'use_k17', False)
    elif cond == 'listed':
        monkeypatch.setattr(S, 'k17_slower', frozenset({(16, 32, 32)}))
    elif cond == 'gradient':
        stem.conv.weight.requires_grad_(True)
    elif cond == 'autocast':
        was = torch.is_autocast_enabled('cuda')
        torch.set_autocast_enabled('cuda', True)
    elif cond == 'odd_shape':
        x = x[:, :, :31, :28].contiguous()
    elif cond == 'layout':
        x = torch.rand(2, 3, 32, 64, generator=cases.gen(4))[:, :, :, ::2]
    try:
        with grad:
            assert not stem.k17_takes(x)
            if cond == 'decision_changed':
                # Preproc is told "yes" and hands x over untouched; by the time the stem runs, the answer is "no"
                monkeypatch.setattr(stem, 'k17_takes', lambda t: True)
                handed = pre(x)
                assert handed is x and stem._handed is x
                monkeypatch.undo()
            else:
                assert pre(x) is not x and stem._handed is None   # Preproc itself takes the branch of before
                stem.hand_over(x)                                  # ... and if it had handed x over all the same:
                handed = x
            want = plain_stem(x * 2 - 1)
            got = stem(handed)
    finally:
        if cond == 'autocast':
            torch.set_autocast_enabled('cuda', was)
    assert stem.last_path == 'library' and stem._handed is None
    assert len(spy.seen) == 1 and torch.equal(spy.seen[0], x * 2 - 1)
    assert torch.equal(got, want)
    # a tensor that was NOT handed over comes preprocessed already: it is convolved as it is, once
    stem.hand_over(x)
    y = (x * 2 - 1).detach()
    with torch.no_grad():
        stem(y)
    assert torch.equal(spy.seen[-1], y) and stem._handed is None


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


def test_loaders_pass_fuse_stem_through(tmp_path):
    import inspect
    from metrabs_amd import backbones, loading
    for fn in (loading.load_crop_model, loading.load_multiperson_model, backbones.fold_batchnorm):
        assert inspect.signature(fn).parameters['fuse_stem'].default is False
    d = _model_dir(tmp_path)
    default = loading.load_crop_model(d, dtype=torch.float16)
    assert not _armed_parts(default.backbone)[1]
    for dtype, want in ((None, torch.float32), (torch.float32, torch.float32), (torch.float16, torch.float16),
                        (torch.bfloat16, torch.bfloat16)):
        m = loading.load_crop_model(d, dtype=dtype, fuse_stem=True)   # dtype=None too: an f32 folded copy
        (pre,), (stem,) = _armed_parts(m.backbone)
        assert stem.conv.weight.dtype == want and pre.hand_to == (stem,)
        assert not any(isinstance(k, torch.nn.BatchNorm2d) for k in m.backbone.modules())
    assert list(loading.load_crop_model(d, dtype=torch.float16, fuse_stem=True).state_dict()) == \
        list(default.state_dict())
    m = loading.load_crop_model(d, dtype=torch.float16, fuse_stem=True, fuse_blocks=True)
    assert _armed_parts(m.backbone)[1] and any(k.fused_pair for k in m.backbone.modules()
                                               if isinstance(k, backbones.FusedMBConv))

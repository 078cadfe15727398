"""CPU: the host side of K19 (csrc/conv3x3_winograd.hip): the weight transform, the shape query, the entry's refusals
(every check is made before anything is enqueued, so they need no GPU), and the module side -- what
fold_batchnorm(winograd3x3=True) arms per backbone, its argument rule, unchanged keys, and the armed copy on the CPU,
where it takes the torch ops like the copy without the option."""
import ctypes
import inspect

import pytest
import torch

F16, BF16 = torch.float16, torch.bfloat16
ARMED = {'efficientnetv2-s': 8, 'efficientnetv2-l': 16, 'resnet18': 13, 'mobilenetv3': 0}


def _net(name):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    return backbones.build_backbone(name).eval()


def _formula(w):
    """U = G g G^T in fp64, written out entry by entry, rounded to f32 once: [16, Cout, Cin]."""
    g = w.double()
    rows = [lambda a: a[..., 0, :], lambda a: 0.5 * (a[..., 0, :] + a[..., 1, :] + a[..., 2, :]),
            lambda a: 0.5 * (a[..., 0, :] - a[..., 1, :] + a[..., 2, :]), lambda a: a[..., 2, :]]
    out = []
    for i in range(4):
        gi = rows[i](g)                      # [Cout, Cin, 3]: row i of G g
        cols = [gi[..., 0], 0.5 * (gi[..., 0] + gi[..., 1] + gi[..., 2]), 0.5 * (gi[..., 0] - gi[..., 1] + gi[..., 2]),
                gi[..., 2]]
        out += cols
    return torch.stack(out).float()


def test_pack_is_the_fp64_formula_rounded_once():
    from metrabs_amd import kernels
    g = torch.Generator().manual_seed(1)
    w = torch.randn(24, 8, 3, 3, generator=g) / 72 ** 0.5
    u = kernels.pack_conv3x3_winograd_weight(w)
    assert u.shape == (16, 24, 8) and u.dtype == torch.float32 and u.is_contiguous()
    assert torch.equal(u, _formula(w))
    # multiples of 4: every entry of G g G^T is an integer, so the transform is exact in any precision
    wi = 4.0 * torch.randint(-2, 3, (5, 12, 3, 3), generator=g).float()
    ui = kernels.pack_conv3x3_winograd_weight(wi)
    assert torch.equal(ui, _formula(wi)) and torch.equal(ui, ui.round())
    G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])
    assert torch.equal(ui.view(4, 4, 5, 12).permute(2, 3, 0, 1), G @ wi @ G.t())   # exact in f32 too
    # xi = 4 i + j: the corners are the weight's own corners
    assert torch.equal(u[0], w[:, :, 0, 0]) and torch.equal(u[3], w[:, :, 0, 2]) and torch.equal(u[15], w[:, :, 2, 2])
    with pytest.raises(ValueError):
        kernels.pack_conv3x3_winograd_weight(w[:, :, :2])
    with pytest.raises(ValueError):
        kernels.pack_conv3x3_winograd_weight(w.half())


def _armed_shapes(name, res):
    """(Cin, Cout, H, W) of every armed layer's input at `res` px, from a hooked CPU forward."""
    from metrabs_amd import backbones
    net = backbones.fold_batchnorm(_net(name), fused_epilogue=True, winograd3x3=True)
    shapes = set()

    def hook(mod, args):
        shapes.add((args[0].shape[1], mod.conv.out_channels, args[0].shape[2], args[0].shape[3]))

    hs = [m.register_forward_pre_hook(hook) for m in net.modules()
          if isinstance(m, backbones.WinogradConv3x3BiasAct)]
    assert len(hs) == ARMED[name]
    with torch.inference_mode():
        net(torch.rand(1, 3, res, res))
    for h in hs:
        h.remove()
    return sorted(shapes)


@pytest.mark.parametrize('name,res', [('efficientnetv2-s', 256), ('efficientnetv2-s', 224), ('efficientnetv2-s', 160),
                                      ('resnet18', 256), ('resnet18', 224), ('resnet18', 160),
                                      ('efficientnetv2-l', 384)])
def test_lds_bytes_is_nonzero_for_every_armed_shape(name, res, hip_lib):
    shapes = _armed_shapes(name, res)
    assert len(shapes) >= 3
    for (K, M, H, W) in shapes:
        for B in (1, 3, 64):
            if H % 2 == 0 and W % 4 == 0:
                assert hip_lib.mtr_conv3x3_winograd_lds_bytes(B, K, M, H, W) == 16 * 8 * (80 + 48) * 4, (K, M, H, W)
            else:   # (ResNet-18's 7x7, 5x5 and 10x10 maps at 224 / 160 px: the library path)
                assert hip_lib.mtr_conv3x3_winograd_lds_bytes(B, K, M, H, W) == 0, (K, M, H, W)
    if res in (256, 384):
        assert all(H % 2 == 0 and W % 4 == 0 for (_, _, H, W) in shapes)


def test_lds_bytes_is_zero_for_what_the_entry_refuses(hip_lib):
    q = hip_lib.mtr_conv3x3_winograd_lds_bytes
    assert q(1, 8, 8, 8, 8) > 0 and q(1, 4, 1, 2, 4) > 0
    assert q(1, 8, 8, 7, 8) == 0          # odd H
    assert q(1, 8, 8, 8, 6) == 0          # W % 4 != 0
    assert q(1, 8, 8, 8, 7) == 0
    assert q(1, 6, 8, 8, 8) == 0          # Cin % 4 != 0
    assert q(1, 3, 8, 8, 8) == 0
    for bad in ((0, 8, 8, 8, 8), (-1, 8, 8, 8, 8), (1, 0, 8, 8, 8), (1, 8, 0, 8, 8), (1, 8, 8, 0, 8),
                (1, 8, 8, 8, 0), (1, -4, 8, 8, 8), (1, 8, 8, -2, 8), (1, 8, 8, 8, -4)):
        assert q(*bad) == 0, bad
    assert q(1, 8, 8, 32768, 32768) == 0          # Cin H W past 2^31
    assert q(2 ** 22, 8, 8, 64, 64) == 0          # the batch's tiles past 2^31


def test_entry_refusals_need_no_gpu(hip_lib):
    """Every call is refused on the host before anything is enqueued: the buffers are host memory."""
    f = hip_lib.mtr_conv3x3_winograd_bias_act
    buf = (ctypes.c_float * 8192)()
    out = (ctypes.c_float * 8192)()
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    obase = ctypes.addressof(out) + (-ctypes.addressof(out)) % 16
    p, q, null = ctypes.c_void_p(base), ctypes.c_void_p(obase), ctypes.c_void_p(0)
    # f(x, weight_u, bias, residual, act, B, Cin, Cout, H, W, y, stream)
    assert f(null, p, p, null, 0, 1, 8, 8, 8, 8, q, null) == -1      # MTR_E_NULL
    assert f(p, null, p, null, 0, 1, 8, 8, 8, 8, q, null) == -1
    assert f(p, p, null, null, 0, 1, 8, 8, 8, 8, q, null) == -1
    assert f(p, p, p, null, 0, 1, 8, 8, 8, 8, null, null) == -1
    assert f(p, p, p, null, 0, 1, 8, 8, 7, 8, q, null) == -2         # MTR_E_SHAPE: odd H
    assert f(p, p, p, null, 0, 1, 8, 8, 8, 6, q, null) == -2         # W % 4
    assert f(p, p, p, null, 0, 1, 6, 8, 8, 8, q, null) == -2         # Cin % 4
    assert f(p, p, p, null, 0, 1, 8, 0, 8, 8, q, null) == -2
    assert f(p, p, p, null, 0, -1, 8, 8, 8, 8, q, null) == -2
    assert f(p, p, p, null, 4, 1, 8, 8, 8, 8, q, null) == -4         # MTR_E_PARAM: act code
    assert f(p, p, p, null, -1, 1, 8, 8, 8, 8, q, null) == -4
    assert f(p, p, p, null, 0, 1, 8, 8, 8, 8, p, null) == -4         # y is x
    assert f(p, p, p, q, 0, 1, 8, 8, 8, 8, q, null) == -4            # y is the residual
    inside = ctypes.c_void_p(base + 256)
    assert f(p, p, p, null, 0, 1, 8, 8, 8, 8, inside, null) == -4    # y overlaps x
    assert f(inside, p, p, p, 0, 1, 8, 8, 8, 8, ctypes.c_void_p(base + 512), null) == -4
    odd = ctypes.c_void_p(base + 8)
    assert f(odd, p, p, null, 0, 1, 8, 8, 8, 8, q, null) == -6       # MTR_E_ALIGN: x, weight, y, residual
    assert f(p, odd, p, null, 0, 1, 8, 8, 8, 8, q, null) == -6
    assert f(p, p, p, null, 0, 1, 8, 8, 8, 8, ctypes.c_void_p(obase + 8), null) == -6
    assert f(p, p, p, odd, 0, 1, 8, 8, 8, 8, q, null) == -6
    assert f(p, p, p, null, 0, 0, 8, 8, 8, 8, q, null) == 0          # B = 0: nothing to do, no launch
    assert all(v == 0.0 for v in out)


def test_option_is_off_by_default_and_needs_an_f32_fused_copy():
    from metrabs_amd import backbones, loading
    for fn in (backbones.fold_batchnorm, loading.load_crop_model, loading.load_multiperson_model):
        assert inspect.signature(fn).parameters['winograd3x3'].default is False
    net = _net('efficientnetv2-s')
    with pytest.raises(ValueError, match='winograd3x3'):
        backbones.fold_batchnorm(net, winograd3x3=True)
    with pytest.raises(ValueError, match='winograd3x3'):
        backbones.fold_batchnorm(net, fused_epilogue=False, winograd3x3=True)
    for dtype in (F16, BF16):
        with pytest.raises(ValueError, match='winograd3x3'):
            backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, winograd3x3=True)
    c = backbones.fold_batchnorm(net, fused_epilogue=True, winograd3x3=True, fuse_stem=True, block_depthwise=True)
    assert sum(isinstance(m, backbones.WinogradConv3x3BiasAct) for m in c.modules()) == 8   # independent of the others
    assert any(isinstance(m, backbones.StemConvBiasAct) for m in c.modules())


@pytest.mark.parametrize('name', list(ARMED))
def test_what_is_armed_keys_and_the_cpu_path(name):
    from metrabs_amd import backbones
    W3 = backbones.WinogradConv3x3BiasAct
    net = _net(name)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, winograd3x3=True)
    assert not any(isinstance(m, W3) for m in plain.modules())
    mods = [m for m in armed.modules() if isinstance(m, W3)]
    assert len(mods) == ARMED[name]
    for m in mods:
        c = m.conv
        assert c.kernel_size == (3, 3) and c.stride == (1, 1) and c.padding == (1, 1) and c.groups == 1
        assert c.in_channels % 4 == 0 and not m.emit_mean and c.weight.shape[2:] == (3, 3)   # the OIHW weight is kept
    # every other dense 3x3 ConvBiasAct is one the option does not cover
    for m in armed.modules():
        if type(m) is backbones.ConvBiasAct and m.conv.kernel_size == (3, 3) and m.conv.groups == 1:
            assert m.conv.stride != (1, 1) or m.conv.in_channels % 4 or m.conv.padding != (1, 1) or m.emit_mean
    assert list(armed.state_dict()) == list(plain.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(armed.state_dict().values(), plain.state_dict().values()))
    # the pre_pair arming of the f32 copy happens for the subclass too
    pre = lambda n: [bool(m.pre_pair) for m in n.modules() if isinstance(m, backbones.FusedMBConv)]
    assert pre(armed) == pre(plain)
    if name.startswith('efficientnet'):
        blocks = [m for m in armed.modules() if isinstance(m, backbones.FusedMBConv) and m.pre_pair]
        assert blocks and sum(isinstance(m.pre_pair[0], W3) for m in blocks) == ARMED[name] - (2 if name[-1] == 's' else 4)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    with torch.inference_mode():
        a, p = armed(x), plain(x)
    assert torch.equal(a, p)
    assert all(m.last_path == 'library' for m in mods)
    assert not any(getattr(m, 'last_path', None) == 'k19' for m in armed.modules())


def test_loaders_pass_winograd3x3_through(tmp_path):
    import numpy as np
    from oracle import cases
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
    m = loading.load_crop_model(d, winograd3x3=True)   # always the folded copy with fused epilogues
    assert sum(isinstance(k, backbones.WinogradConv3x3BiasAct) for k in m.backbone.modules()) == 8
    assert list(m.state_dict()) == list(loading.load_crop_model(d, fold_batchnorm=True, fused_epilogue=True).state_dict())
    m = loading.load_crop_model(d, dtype=torch.float32, winograd3x3=True)
    assert sum(isinstance(k, backbones.WinogradConv3x3BiasAct) for k in m.backbone.modules()) == 8
    assert not any(isinstance(k, backbones.WinogradConv3x3BiasAct) for k in loading.load_crop_model(d).backbone.modules())
    for dtype in (F16, BF16):
        with pytest.raises(ValueError, match='winograd3x3'):
            loading.load_crop_model(d, dtype=dtype, winograd3x3=True)

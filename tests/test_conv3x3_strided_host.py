"""CPU: the host side of K22 (csrc/conv3x3_strided.hip): the weight permutation, the shape query, the entry's refusals
(every check is made before anything is enqueued, so they need no GPU -- the activation-code refusal of this entry,
whose parameter is named act_code, is pinned HERE and not in test_act_code_refusals.py), and the module side -- what
fold_batchnorm(strided3x3=True) arms per backbone, its argument rule, unchanged keys, references that stay inside the
tree with every f32 option on, and the armed copy on the CPU, where it takes the torch ops like the default copy."""
import ctypes
import inspect

import pytest
import torch

from test_backbone_option_combos_host import stale_references

F16, BF16 = torch.float16, torch.bfloat16
ARMED = {'efficientnetv2-s': 2, 'efficientnetv2-l': 2, 'mobilenetv3': 0, 'resnet18': 3}
ALL_F32 = dict(fuse_stem=True, block_depthwise=True, winograd3x3=True, split_gemm=True, strided3x3=True)


def _net(name):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    return backbones.build_backbone(name).eval()


def test_option_is_off_by_default_and_needs_an_f32_fused_copy():
    from metrabs_amd import backbones, loading
    for fn in (backbones.fold_batchnorm, loading.load_crop_model, loading.load_multiperson_model):
        assert inspect.signature(fn).parameters['strided3x3'].default is False
    net = _net('efficientnetv2-s')
    with pytest.raises(ValueError, match='strided3x3'):
        backbones.fold_batchnorm(net, strided3x3=True)                         # without fused_epilogue
    for dtype in (F16, BF16):
        with pytest.raises(ValueError, match='strided3x3'):
            backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, strided3x3=True)
    c = backbones.fold_batchnorm(net, fused_epilogue=True, strided3x3=True, fuse_stem=True, winograd3x3=True)
    assert sum(isinstance(m, backbones.StridedConv3x3BiasAct) for m in c.modules()) == 2   # independent of the others
    assert sum(isinstance(m, backbones.WinogradConv3x3BiasAct) for m in c.modules()) == 8
    assert any(isinstance(m, backbones.StemConvBiasAct) for m in c.modules())


@pytest.mark.parametrize('name', list(ARMED))
def test_what_is_armed_keys_references_and_the_cpu_path(name):
    from metrabs_amd import backbones
    S3 = backbones.StridedConv3x3BiasAct
    net = _net(name)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, strided3x3=True)
    every = backbones.fold_batchnorm(net, fused_epilogue=True, **ALL_F32)
    assert not any(isinstance(m, S3) for m in plain.modules())
    for copy in (armed, every):
        mods = [m for m in copy.modules() if isinstance(m, S3)]
        assert len(mods) == ARMED[name]
        for m in mods:
            c = m.conv
            assert c.kernel_size == (3, 3) and c.stride == (2, 2) and c.padding == (1, 1) and c.groups == 1
            assert c.in_channels % 4 == 0 and not m.emit_mean and c.weight.shape[2:] == (3, 3)   # the OIHW weight stays
        assert list(copy.state_dict()) == list(plain.state_dict())
        assert all(torch.equal(a, b) for a, b in zip(copy.state_dict().values(), plain.state_dict().values()))
        # every pre_pair holds the block's own two layers, and no reference points outside the tree
        assert stale_references(copy) == []
        for blk in copy.modules():
            if isinstance(blk, backbones.FusedMBConv) and blk.pre_pair:
                assert blk.pre_pair[0] is blk.block[0][0] and blk.pre_pair[1] is blk.block[1][0]
        pre = lambda n: [bool(m.pre_pair) for m in n.modules() if isinstance(m, backbones.FusedMBConv)]
        assert pre(copy) == pre(plain)
    if name.startswith('efficientnet'):   # both armed layers are the expands of stride-2 FusedMBConv blocks
        blocks = [m for m in armed.modules() if isinstance(m, backbones.FusedMBConv) and m.pre_pair]
        assert sum(isinstance(m.pre_pair[0], S3) for m in blocks) == 2
    # the stem (Cin = 3) is not this option's
    stems = [m for m in armed.modules() if isinstance(m, backbones.ConvBiasAct) and m.conv.in_channels == 3]
    assert stems and not any(isinstance(m, S3) for m in stems)
    x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    with torch.inference_mode():
        a, p = armed(x), plain(x)
    assert torch.equal(a, p)
    assert all(m.last_path == 'library' for m in armed.modules() if isinstance(m, S3))
    assert not any(getattr(m, 'last_path', None) == 'k22' for m in armed.modules())


def test_pack_is_a_permutation():
    from metrabs_amd import kernels
    g = torch.Generator().manual_seed(1)
    w = torch.randn(20, 12, 3, 3, generator=g)
    p = kernels.pack_conv3x3_strided_weight(w)
    assert p.shape == (3, 20, 3, 3, 4) and p.dtype == torch.float32 and p.is_contiguous()
    assert torch.equal(p.flatten().sort().values, w.flatten().sort().values)
    # the inverse gather: element (c4, m, ky, kx, j) is w[m, 4 c4 + j, ky, kx]
    c4, m, ky, kx, j = torch.meshgrid(torch.arange(3), torch.arange(20), torch.arange(3), torch.arange(3),
                                      torch.arange(4), indexing='ij')
    back = torch.empty_like(w)
    back[m, 4 * c4 + j, ky, kx] = p
    assert torch.equal(back, w)
    assert float(p[2, 7, 1, 2, 3]) == float(w[7, 11, 1, 2])
    with pytest.raises(ValueError):
        kernels.pack_conv3x3_strided_weight(w.half())
    with pytest.raises(ValueError):
        kernels.pack_conv3x3_strided_weight(w.double())
    with pytest.raises(ValueError):
        kernels.pack_conv3x3_strided_weight(w[:, :, :2])
    with pytest.raises(ValueError):
        kernels.pack_conv3x3_strided_weight(w[:, :, 0])
    with pytest.raises(ValueError):
        kernels.pack_conv3x3_strided_weight(w[:, :6])          # Cin % 4 != 0: no layer the option arms


def test_weight_s_is_derived_state():
    from metrabs_amd import backbones, kernels
    armed = backbones.fold_batchnorm(_net('resnet18'), fused_epilogue=True, strided3x3=True)
    m = next(k for k in armed.modules() if isinstance(k, backbones.StridedConv3x3BiasAct))
    keys = list(armed.state_dict())
    a = m.weight_s()
    assert a is m.weight_s() and torch.equal(a, kernels.pack_conv3x3_strided_weight(m.conv.weight))
    assert list(armed.state_dict()) == keys and not any(b is a for b in armed.buffers())
    with torch.no_grad():
        m.conv.weight.mul_(2.0)                                  # written in place: made anew
    assert torch.equal(m.weight_s(), kernels.pack_conv3x3_strided_weight(m.conv.weight))


def test_lds_bytes_is_zero_for_what_the_entry_refuses(hip_lib):
    q = hip_lib.mtr_conv3x3s2_lds_bytes
    assert q(1, 4, 5, 8, 8) > 0 and q(64, 48, 192, 64, 64) > 0 and q(3, 256, 512, 16, 16) > 0
    assert q(1, 6, 5, 8, 8) == 0          # K = 6: Cin % 4 != 0
    assert q(1, 4, 5, 7, 8) == 0          # H = 7: an odd map
    assert q(1, 4, 5, 8, 12) == 0         # W = 12: (W / 2) % 4 != 0
    assert q(1, 4, 5, 8, 7) == 0
    for bad in ((0, 4, 5, 8, 8), (-1, 4, 5, 8, 8), (1, 0, 5, 8, 8), (1, 4, 0, 8, 8), (1, 4, 5, 0, 8), (1, 4, 5, 8, 0),
                (1, -4, 5, 8, 8), (1, 4, 5, -2, 8), (1, 4, 5, 8, -8)):
        assert q(*bad) == 0, bad
    assert q(1, 8, 8, 32768, 32768) == 0          # Cin H W past 2^31
    assert q(2 ** 31, 4, 5, 8, 8) == 0            # the grid past 2^31


def test_entry_refusals_need_no_gpu(hip_lib):
    """Every call is refused on the host before anything is enqueued: the buffers are host memory."""
    f = hip_lib.mtr_conv3x3s2_bias_act
    buf = (ctypes.c_float * 8192)()
    out = (ctypes.c_float * 8192)()
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    obase = ctypes.addressof(out) + (-ctypes.addressof(out)) % 16
    p, q, null = ctypes.c_void_p(base), ctypes.c_void_p(obase), ctypes.c_void_p(0)
    # f(x, w_packed, bias, residual, act_code, B, Cin, Cout, H, W, y, stream)
    assert f(null, p, p, null, 0, 1, 4, 5, 8, 8, q, null) == -1      # MTR_E_NULL
    assert f(p, null, p, null, 0, 1, 4, 5, 8, 8, q, null) == -1
    assert f(p, p, null, null, 0, 1, 4, 5, 8, 8, q, null) == -1
    assert f(p, p, p, null, 0, 1, 4, 5, 8, 8, null, null) == -1
    assert f(null, null, null, null, 9, 1, 6, 5, 7, 12, null, null) == -1   # NULL comes first
    assert f(p, p, p, null, 0, 1, 6, 5, 8, 8, q, null) == -2         # MTR_E_SHAPE: K = 6
    assert f(p, p, p, null, 0, 1, 4, 5, 7, 8, q, null) == -2         # H = 7
    assert f(p, p, p, null, 0, 1, 4, 5, 8, 12, q, null) == -2        # W = 12
    assert f(p, p, p, null, 0, 1, 4, 0, 8, 8, q, null) == -2
    assert f(p, p, p, null, 0, -1, 4, 5, 8, 8, q, null) == -2
    for code in (-1, 4):                                             # MTR_E_PARAM: the activation code, B = 1 and B = 0
        assert f(p, p, p, null, code, 1, 4, 5, 8, 8, q, null) == -4
        assert f(p, p, p, null, code, 0, 4, 5, 8, 8, q, null) == -4
    assert [f(p, p, p, null, code, 0, 4, 5, 8, 8, q, null) for code in range(4)] == [0] * 4   # B = 0: nothing to do
    assert f(p, p, p, null, 0, 1, 4, 5, 8, 8, p, null) == -4         # y is x
    assert f(p, p, p, q, 0, 1, 4, 5, 8, 8, q, null) == -4            # y is the residual
    inside = ctypes.c_void_p(base + 256)
    assert f(p, p, p, null, 0, 1, 4, 5, 8, 8, inside, null) == -4    # y overlaps x
    assert f(inside, p, p, p, 0, 1, 4, 5, 8, 8, ctypes.c_void_p(base + 128), null) == -4   # y overlaps the residual
    odd = ctypes.c_void_p(base + 8)
    assert f(odd, p, p, null, 0, 1, 4, 5, 8, 8, q, null) == -6       # MTR_E_ALIGN: x, weight, y, residual
    assert f(p, odd, p, null, 0, 1, 4, 5, 8, 8, q, null) == -6
    assert f(p, p, p, null, 0, 1, 4, 5, 8, 8, ctypes.c_void_p(obase + 8), null) == -6
    assert f(p, p, p, odd, 0, 1, 4, 5, 8, 8, q, null) == -6
    assert all(v == 0.0 for v in out)


def test_loaders_pass_strided3x3_through(tmp_path):
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
    S3 = backbones.StridedConv3x3BiasAct
    m = loading.load_crop_model(d, strided3x3=True)   # always the folded copy with fused epilogues
    assert sum(isinstance(k, S3) for k in m.backbone.modules()) == 2
    assert list(m.state_dict()) == list(loading.load_crop_model(d, fold_batchnorm=True, fused_epilogue=True).state_dict())
    m = loading.load_crop_model(d, dtype=torch.float32, strided3x3=True)
    assert sum(isinstance(k, S3) for k in m.backbone.modules()) == 2
    assert not any(isinstance(k, S3) for k in loading.load_crop_model(d).backbone.modules())
    for dtype in (F16, BF16):
        with pytest.raises(ValueError, match='strided3x3'):
            loading.load_crop_model(d, dtype=dtype, strided3x3=True)

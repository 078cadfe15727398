"""CPU: the host side of K20 (csrc/conv1x1_split.hip): the weight split, the shape query, and the module side -- what
fold_batchnorm(split_gemm=True) arms per backbone, its argument rule, unchanged keys, the armed copy on the CPU (where
K20 takes nothing), and the loaders."""
import inspect

import pytest
import torch

F16, BF16 = torch.float16, torch.bfloat16
NAMES = ['efficientnetv2-s', 'efficientnetv2-l', 'mobilenetv3', 'resnet18']


def _net(name):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    return backbones.build_backbone(name).eval()


@pytest.mark.parametrize('K', [24, 200, 960])
def test_pack_splits_into_three_bf16_pieces_that_sum_back(K):
    from metrabs_amd import kernels
    g = torch.Generator().manual_seed(K)
    M = 40
    w = torch.randn(M, K, generator=g) / K ** 0.5
    for weight in (w, w.view(M, K, 1, 1)):
        ws = kernels.pack_conv1x1_split_weight(weight)
        Kp = (K + 31) // 32 * 32
        assert ws.shape == (3, M, Kp) and ws.dtype == BF16 and ws.is_contiguous()
        assert not ws[:, :, K:].any()                                   # the zero tail
        w0, w1, w2 = (ws[i, :, :K].float() for i in range(3))
        assert torch.equal(w0 + w1 + w2, w)                             # bit for bit, f32 sums in that order
        assert torch.equal(ws[0, :, :K], w.to(BF16))                    # round to nearest
        assert torch.equal(ws[1, :, :K], (w - w0).to(BF16)) and torch.equal(ws[2, :, :K], (w - w0 - w1).to(BF16))
        assert bool(w1.any()) and bool(w2.any())
        assert float((w1.abs() - 2.0 ** -8 * w.abs()).max()) <= 0 and float((w2.abs() - 2.0 ** -16 * w.abs()).max()) <= 0
    # exact bf16 values: pieces 1 and 2 are all zero
    wb = w.to(BF16).float()
    ws = kernels.pack_conv1x1_split_weight(wb)
    assert torch.equal(ws[0, :, :K].float(), wb) and not ws[1].any() and not ws[2].any()


def test_pack_refuses_other_ranks_and_dtypes():
    from metrabs_amd import kernels
    w = torch.randn(8, 16)
    for bad in (w[0], w.view(8, 16, 1), w.view(8, 4, 2, 2), w.view(1, 8, 16, 1, 1)):
        with pytest.raises(ValueError):
            kernels.pack_conv1x1_split_weight(bad)
    for dtype in (F16, BF16, torch.float64):
        with pytest.raises(ValueError):
            kernels.pack_conv1x1_split_weight(w.to(dtype))


def test_split_supported_answers_on_the_host(hip_lib):
    g = hip_lib.mtr_conv1x1_split_supported
    assert g(1, 8, 8, 16) == 0 and g(64, 160, 960, 256) == 0 and g(3, 1280, 256, 64) == 0
    assert g(1, 8, 8, 49) == -2 and g(1, 8, 8, 18) == -2     # H*W % 4
    assert g(1, 8, 6, 16) == -2 and g(1, 8, 30, 16) == -2    # K % 4
    assert g(-1, 8, 8, 16) == -2                             # B < 0
    assert g(0, 8, 8, 16) == 0                               # B = 0: the entry returns MTR_OK without a launch
    assert g(1, 0, 8, 16) == -2 and g(1, 8, 0, 16) == -2 and g(1, 8, 8, 0) == -2
    assert g(2 ** 20, 8, 8, 4096) == -2                      # B * HW past 2^31


def test_option_is_off_by_default_and_needs_an_f32_fused_copy():
    from metrabs_amd import backbones, loading
    for fn in (backbones.fold_batchnorm, loading.load_crop_model, loading.load_multiperson_model):
        assert inspect.signature(fn).parameters['split_gemm'].default is False
    net = _net('mobilenetv3')
    with pytest.raises(ValueError, match='split_gemm'):
        backbones.fold_batchnorm(net, split_gemm=True)
    with pytest.raises(ValueError, match='split_gemm'):
        backbones.fold_batchnorm(net, fused_epilogue=False, split_gemm=True)
    for dtype in (F16, BF16):
        with pytest.raises(ValueError, match='split_gemm'):
            backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, split_gemm=True)
    # independent of the other options
    c = backbones.fold_batchnorm(net, fused_epilogue=True, split_gemm=True, fuse_stem=True, block_depthwise=True)
    d = backbones.fold_batchnorm(net, fused_epilogue=True, split_gemm=True)
    armed = lambda n: sum(bool(getattr(m, 'split_gemm', False)) for m in n.modules())
    assert armed(c) == armed(d) > 0 and any(isinstance(m, backbones.StemConvBiasAct) for m in c.modules())


def _is_1x1_s1_meanless(m):
    from metrabs_amd import backbones
    if not isinstance(m, backbones.ConvBiasAct):
        return False
    c = m.conv
    return (c.kernel_size == (1, 1) and c.stride == (1, 1) and c.padding == (0, 0) and c.groups == 1
            and not m.emit_mean)


@pytest.mark.parametrize('name', NAMES)
def test_what_is_armed_keys_and_the_cpu_path(name):
    from metrabs_amd import backbones
    net = _net(name)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, split_gemm=True)
    assert not any(getattr(m, 'split_gemm', False) for m in plain.modules())
    mods = [m for m in armed.modules() if getattr(m, 'split_gemm', False)]
    assert len(mods) == sum(_is_1x1_s1_meanless(m) for m in armed.modules())
    assert all(_is_1x1_s1_meanless(m) for m in mods)
    assert (len(mods) > 0) == (name != 'resnet18')       # (ResNet-18's 1x1 convolutions are its stride-2 shortcuts)
    assert backbones.ConvBiasAct.split_gemm is False and backbones.ConvBiasAct.use_k20 is True
    assert isinstance(backbones.ConvBiasAct.k20_slower, frozenset)
    assert [type(m) for m in armed.modules()] == [type(m) for m in plain.modules()]
    assert list(armed.state_dict()) == list(plain.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(armed.state_dict().values(), plain.state_dict().values()))
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    with torch.inference_mode():
        a, p = armed(x), plain(x)
    assert torch.equal(a, p)                               # K20 takes no CPU tensor
    assert all(m.last_path == 'library' and not m.k20_takes(x) for m in mods)
    assert not any(str(getattr(m, 'last_path', None)).startswith('k20') for m in armed.modules())
    assert all(m._ws is None for m in mods)                # nothing was packed for a path that did not run


def test_loaders_pass_split_gemm_through(tmp_path):
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
    armed = lambda m: sum(bool(getattr(k, 'split_gemm', False)) for k in m.backbone.modules())
    m = loading.load_crop_model(d, split_gemm=True)   # always the folded copy with fused epilogues
    n = armed(m)
    assert n == sum(_is_1x1_s1_meanless(k) for k in m.backbone.modules()) > 0
    assert list(m.state_dict()) == list(loading.load_crop_model(d, fold_batchnorm=True, fused_epilogue=True).state_dict())
    assert armed(loading.load_crop_model(d, dtype=torch.float32, split_gemm=True)) == n
    assert armed(loading.load_crop_model(d, split_gemm=True, winograd3x3=True)) == n
    assert armed(loading.load_crop_model(d)) == 0
    assert armed(loading.load_crop_model(d, fold_batchnorm=True, fused_epilogue=True)) == 0
    for dtype in (F16, BF16):
        with pytest.raises(ValueError, match='split_gemm'):
            loading.load_crop_model(d, dtype=dtype, split_gemm=True)
        with pytest.raises(ValueError, match='split_gemm'):
            loading.load_multiperson_model(d, device='cpu', dtype=dtype, split_gemm=True)

"""CPU: the host side of K21 (csrc/conv3x3_split.hip): the weight split, the shape query, the entry's refusals (every
check is made before anything is enqueued, so they need no GPU -- the activation-code refusal of this entry, whose
parameter is named act_code, is pinned HERE and not in test_act_code_refusals.py), a restatement of the six-product
sum on the exact-integer cases the GPU test runs, and the module side -- what fold_batchnorm(split3x3=True) arms per
backbone, its argument rule, unchanged keys, references that stay inside the tree with every f32 option on, the
combination with winograd3x3, and the armed copy on the CPU, where it takes the torch ops like the default copy."""
import ctypes
import inspect

import pytest
import torch
import torch.nn.functional as F

from test_backbone_option_combos_host import stale_references

F16, BF16 = torch.float16, torch.bfloat16
ARMED = {'efficientnetv2-s': 8, 'efficientnetv2-l': 16, 'mobilenetv3': 0, 'resnet18': 13}
ALL_F32 = dict(fuse_stem=True, block_depthwise=True, winograd3x3=True, split_gemm=True, strided3x3=True,
               split3x3=True)
# (w piece, x piece) of the six products K21 sums, in its order
PRODUCTS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))
INT_SHAPES = ((2, 40, 24, 8, 12), (1, 136, 72, 4, 8))


def _net(name):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    return backbones.build_backbone(name).eval()


# ---- the exact-integer cases (shared with tests/test_gpu_conv3x3_split.py)

def _odd_ints(shape, bits, g):
    """Odd integers with exactly `bits` significant bits (top and bottom bit set), of random sign, as f32."""
    v = torch.randint(0, 2 ** (bits - 2), shape, generator=g) * 2 + 1 + 2 ** (bits - 1)
    return (v * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).float()


def _spread(n, C):
    """n channels spread over [0, C): different chunks of 16 and different 8-channel lane groups."""
    return sorted({(i * (C - 1)) // (n - 1) for i in range(n)})


def integer_case(kind, shape, seed=0):
    """-> x [B, Cin, H, W], w [Cout, Cin, 3, 3], bias [Cout], skip [B, Cout, H, W]: f32 tensors of integers whose
    convolution, every partial sum of piece products included, stays below 2^24 in magnitude: K21 must return the fp64
    convolution bit for bit.
    'a': x odd 19-bit (three bf16 pieces) on a lattice of every third row and column -- one per 3x3 window -- on ten
         channels, w in -3..3: needs the products (w0, v0), (w0, v1), (w0, v2).
    'b': the mirror: w odd 19-bit at ONE tap per output channel, (m % 3, (m // 3) % 3), on ten input channels, x in
         -3..3: needs (w0, v0), (w1, v0), (w2, v0).
    'c': both odd 11-bit (two pieces each), x on the lattice at three channels: needs (w1, v1)."""
    B, Cin, Cout, H, W = shape
    g = torch.Generator().manual_seed(1000 * seed + ord(kind))
    small = lambda s: torch.randint(-3, 4, s, generator=g).float()
    x, w = torch.zeros(B, Cin, H, W), torch.zeros(Cout, Cin, 3, 3)
    if kind == 'a':
        ch = _spread(10, Cin)
        x[:, ch, 1::3, 1::3] = _odd_ints((B, len(ch), len(range(1, H, 3)), len(range(1, W, 3))), 19, g)
        w = small((Cout, Cin, 3, 3))
    elif kind == 'b':
        ch = _spread(10, Cin)
        big = _odd_ints((Cout, len(ch)), 19, g)
        for m in range(Cout):
            w[m, ch, m % 3, (m // 3) % 3] = big[m]
        x = small((B, Cin, H, W))
    else:
        ch = _spread(3, Cin)
        x[:, ch, 1::3, 1::3] = _odd_ints((B, len(ch), len(range(1, H, 3)), len(range(1, W, 3))), 11, g)
        w = _odd_ints((Cout, Cin, 3, 3), 11, g)
    bias = torch.randint(-64, 65, (Cout,), generator=g).float()
    skip = torch.randint(-1000, 1001, (B, Cout, H, W), generator=g).float()
    return x, w, bias, skip


def magnitude_sum(x, w, bias):
    """S = conv(|x|, |w|) + |bias| in fp64: what bounds every partial sum of the convolution."""
    return F.conv2d(x.double().abs(), w.double().abs(), bias.double().abs(), padding=1)


def _pieces(t):
    p0 = t.to(BF16)
    r1 = t - p0.float()
    p1 = r1.to(BF16)
    p2 = (r1 - p1.float()).to(BF16)
    return [p.double() for p in (p0, p1, p2)]


def _six_product_sum(x, w, bias, products=PRODUCTS):
    xp, wp = _pieces(x), _pieces(w)
    out = bias.double().view(1, -1, 1, 1)
    for pw, pv in products:
        out = out + F.conv2d(xp[pv], wp[pw], padding=1)
    return out


def test_six_products_are_exact_on_the_integer_cases_and_each_is_needed():
    shape = INT_SHAPES[0]
    cases = {k: integer_case(k, shape) for k in 'abc'}
    for kind, (x, w, bias, _) in cases.items():
        S = magnitude_sum(x, w, bias)
        print(kind, 'max S', float(S.max()))
        assert S.max() < 2 ** 24
        for t in (x, w):
            assert torch.equal(sum(_pieces(t)), t.double())
        assert torch.equal(_six_product_sum(x, w, bias), F.conv2d(x.double(), w.double(), bias.double(), padding=1))
    for drop in PRODUCTS:
        kept = tuple(p for p in PRODUCTS if p != drop)
        changed = [not torch.equal(_six_product_sum(x, w, bias, kept),
                                   F.conv2d(x.double(), w.double(), bias.double(), padding=1))
                   for x, w, bias, _ in cases.values()]
        assert any(changed), drop
    # three pieces in 'a' and 'b', two in 'c'
    assert _pieces(cases['a'][0])[2].abs().max() > 0 and _pieces(cases['b'][1])[2].abs().max() > 0
    assert _pieces(cases['c'][0])[2].abs().max() == 0 and _pieces(cases['c'][0])[1].abs().max() > 0


# ---- the module side

def test_option_is_off_by_default_and_needs_an_f32_fused_copy():
    from metrabs_amd import backbones, loading
    for fn in (backbones.fold_batchnorm, loading.load_crop_model, loading.load_multiperson_model):
        assert inspect.signature(fn).parameters['split3x3'].default is False
    assert ('split3x3', 'f32') in backbones._OPTION_NEEDS
    net = _net('efficientnetv2-s')
    with pytest.raises(ValueError, match='split3x3'):
        backbones.fold_batchnorm(net, split3x3=True)                         # without fused_epilogue
    for dtype in (F16, BF16):
        with pytest.raises(ValueError, match='split3x3'):
            backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, split3x3=True)


def test_with_winograd3x3_the_layers_are_split_layers_and_winograd_alone_is_unchanged():
    from metrabs_amd import backbones
    S3, W3 = backbones.SplitConv3x3BiasAct, backbones.WinogradConv3x3BiasAct
    assert issubclass(S3, W3)
    net = _net('efficientnetv2-s')
    both = backbones.fold_batchnorm(net, fused_epilogue=True, split3x3=True, winograd3x3=True)
    mods = [m for m in both.modules() if isinstance(m, W3)]
    assert len(mods) == 8 and all(type(m) is S3 and m.winograd for m in mods)
    alone = backbones.fold_batchnorm(net, fused_epilogue=True, split3x3=True)
    mods = [m for m in alone.modules() if isinstance(m, W3)]
    assert len(mods) == 8 and all(type(m) is S3 and not m.winograd for m in mods)
    wino = backbones.fold_batchnorm(net, fused_epilogue=True, winograd3x3=True)
    mods = [m for m in wino.modules() if isinstance(m, W3)]
    assert len(mods) == 8 and all(type(m) is W3 for m in mods)
    assert [type(m) for m in wino.modules()] == \
        [W3 if type(m) is S3 else type(m) for m in both.modules()]
    # on the CPU neither kernel takes anything
    x = torch.zeros(1, 24, 8, 8)
    m = next(k for k in both.modules() if isinstance(k, S3) and k.conv.in_channels == 24)
    assert not m.k21_takes(x) and not m.k19_takes(x) and m.path(x) == 'library'


@pytest.mark.parametrize('name', list(ARMED))
def test_what_is_armed_keys_references_and_the_cpu_path(name):
    from metrabs_amd import backbones
    S3 = backbones.SplitConv3x3BiasAct
    net = _net(name)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, split3x3=True)
    every = backbones.fold_batchnorm(net, fused_epilogue=True, **ALL_F32)
    assert not any(isinstance(m, S3) for m in plain.modules())
    for copy in (armed, every):
        mods = [m for m in copy.modules() if isinstance(m, S3)]
        assert len(mods) == ARMED[name]
        for m in mods:
            c = m.conv
            assert c.kernel_size == (3, 3) and c.stride == (1, 1) and c.padding == (1, 1) and c.groups == 1
            assert c.in_channels % 8 == 0 and not m.emit_mean and c.weight.shape[2:] == (3, 3)   # the OIHW weight stays
        assert list(copy.state_dict()) == list(plain.state_dict())
        assert all(torch.equal(a, b) for a, b in zip(copy.state_dict().values(), plain.state_dict().values()))
        # every pre_pair holds the block's own two layers, and no reference points outside the tree
        assert stale_references(copy) == []
        for blk in copy.modules():
            if isinstance(blk, backbones.FusedMBConv) and blk.pre_pair:
                assert blk.pre_pair[0] is blk.block[0][0] and blk.pre_pair[1] is blk.block[1][0]
        pre = lambda n: [bool(m.pre_pair) for m in n.modules() if isinstance(m, backbones.FusedMBConv)]
        assert pre(copy) == pre(plain)
    if name.startswith('efficientnet'):   # the stride-1 FusedMBConv expands of stages 2 and 3 are armed as pairs
        blocks = [m for m in armed.modules() if isinstance(m, backbones.FusedMBConv) and m.pre_pair]
        assert sum(isinstance(m.pre_pair[0], S3) for m in blocks) > 0
    x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    with torch.inference_mode():
        a, p = armed(x), plain(x)
    assert torch.equal(a, p)
    assert all(m.last_path == 'library' for m in armed.modules() if isinstance(m, S3))
    assert not any(getattr(m, 'last_path', None) in ('k21', 'k19') for m in armed.modules())


def test_pack_layout_zero_tail_and_exact_sum():
    from metrabs_amd import kernels
    g = torch.Generator().manual_seed(1)
    w = torch.randn(20, 24, 3, 3, generator=g) * torch.logspace(-6, 6, 20).view(20, 1, 1, 1)
    p = kernels.pack_conv3x3_split_weight(w)
    assert p.shape == (3, 20, 3, 3, 32) and p.dtype == BF16 and p.is_contiguous()       # Cp = 24 -> 32
    assert not p[..., 24:].any()
    body = p[..., :24].float()                                                           # [3, M, ky, kx, ci]
    assert torch.equal((body[0] + body[1] + body[2]).permute(0, 3, 1, 2), w)             # bit for bit
    assert torch.equal(body[0].permute(0, 3, 1, 2), w.to(BF16).float())
    assert float(p[0, 7, 1, 2, 11]) == float(w[7, 11, 1, 2].to(BF16))
    assert float(body[:, 7, 1, 2, 11].sum()) == float(w[7, 11, 1, 2])
    assert (body[1].abs() <= body[0].abs() * 2.0 ** -8).all() and (body[2].abs() <= body[0].abs() * 2.0 ** -16).all()
    assert kernels.pack_conv3x3_split_weight(w[:, :16]).shape == (3, 20, 3, 3, 16)      # a whole chunk: no tail
    with pytest.raises(ValueError):
        kernels.pack_conv3x3_split_weight(w.half())
    with pytest.raises(ValueError):
        kernels.pack_conv3x3_split_weight(w.double())
    with pytest.raises(ValueError):
        kernels.pack_conv3x3_split_weight(w[:, :, :2])
    with pytest.raises(ValueError):
        kernels.pack_conv3x3_split_weight(w[:, :, 0])
    with pytest.raises(ValueError):
        kernels.pack_conv3x3_split_weight(w[:, :12])           # Cin % 8 != 0: no layer the option arms


def test_weight_split3_is_derived_state():
    from metrabs_amd import backbones, kernels
    armed = backbones.fold_batchnorm(_net('resnet18'), fused_epilogue=True, split3x3=True)
    m = next(k for k in armed.modules() if isinstance(k, backbones.SplitConv3x3BiasAct))
    keys = list(armed.state_dict())
    a = m.weight_split3()
    assert a is m.weight_split3() and torch.equal(a, kernels.pack_conv3x3_split_weight(m.conv.weight))
    assert list(armed.state_dict()) == keys and not any(b is a for b in armed.buffers())
    with torch.no_grad():
        m.conv.weight.mul_(3.0)                                  # written in place: made anew
    assert torch.equal(m.weight_split3(), kernels.pack_conv3x3_split_weight(m.conv.weight))


def test_lds_bytes_is_zero_for_what_the_entry_refuses(hip_lib):
    q = hip_lib.mtr_conv3x3_split_lds_bytes
    assert q(1, 8, 5, 8, 8) > 0 and q(64, 48, 192, 64, 64) > 0 and q(3, 256, 512, 16, 16) > 0
    assert q(64, 512, 512, 8, 8) > 0 and q(1, 8, 5, 5, 4) > 0 and q(1, 4096, 8, 3, 4) > 0   # no refusal for LDS
    assert max(q(1, 8, 5, 5, 4), q(64, 48, 192, 64, 64)) <= 160 * 1024     # inside one CU's LDS
    assert q(1, 12, 5, 8, 8) == 0         # Cin % 8 != 0
    assert q(1, 4, 5, 8, 8) == 0
    assert q(1, 8, 5, 8, 6) == 0          # W % 4 != 0
    assert q(1, 8, 5, 8, 7) == 0
    for bad in ((0, 8, 5, 8, 8), (-1, 8, 5, 8, 8), (1, 0, 5, 8, 8), (1, 8, 0, 8, 8), (1, 8, 5, 0, 8), (1, 8, 5, 8, 0),
                (1, -8, 5, 8, 8), (1, 8, -5, 8, 8), (1, 8, 5, -2, 8), (1, 8, 5, 8, -8)):
        assert q(*bad) == 0, bad
    assert q(1, 8, 8, 32768, 32768) == 0          # Cin H W past 2^31
    assert q(1, 8, 2 ** 30, 4, 4) == 0            # Cout H W past 2^31
    assert q(2 ** 31, 8, 5, 4, 4) == 0            # the batch: elements and the grid past 2^31


def test_entry_refusals_need_no_gpu(hip_lib):
    """Every call is refused on the host before anything is enqueued: the buffers are host memory.  One block per
    error code, in the entry's order: NULL, shape, act_code, alignment, overlap."""
    f = hip_lib.mtr_conv3x3_bias_act_split
    buf = (ctypes.c_float * 8192)()
    out = (ctypes.c_float * 8192)()
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    obase = ctypes.addressof(out) + (-ctypes.addressof(out)) % 16
    p, q, null = ctypes.c_void_p(base), ctypes.c_void_p(obase), ctypes.c_void_p(0)
    odd = ctypes.c_void_p(base + 8)
    # f(x, w_split, bias, residual, act_code, B, Cin, Cout, H, W, y, stream)
    assert f(null, p, p, null, 0, 1, 8, 5, 8, 8, q, null) == -1      # MTR_E_NULL
    assert f(p, null, p, null, 0, 1, 8, 5, 8, 8, q, null) == -1
    assert f(p, p, null, null, 0, 1, 8, 5, 8, 8, q, null) == -1
    assert f(p, p, p, null, 0, 1, 8, 5, 8, 8, null, null) == -1
    assert f(null, null, null, null, 9, 1, 12, 5, 7, 6, null, null) == -1   # NULL comes first
    assert f(p, p, p, null, 0, 1, 12, 5, 8, 8, q, null) == -2        # MTR_E_SHAPE: Cin = 12
    assert f(p, p, p, null, 0, 1, 8, 5, 8, 6, q, null) == -2         # W = 6
    assert f(p, p, p, null, 0, 1, 8, 0, 8, 8, q, null) == -2
    assert f(p, p, p, null, 0, 1, 8, 5, 0, 8, q, null) == -2
    assert f(p, p, p, null, 0, -1, 8, 5, 8, 8, q, null) == -2
    assert f(odd, p, p, null, 9, 1, 12, 5, 8, 8, p, null) == -2      # the shape comes before the rest
    for code in (-1, 4):                                             # MTR_E_PARAM: the activation code, B = 1 and B = 0
        assert f(p, p, p, null, code, 1, 8, 5, 8, 8, q, null) == -4
        assert f(p, p, p, null, code, 0, 8, 5, 8, 8, q, null) == -4
    assert [f(p, p, p, null, code, 0, 8, 5, 8, 8, q, null) for code in range(4)] == [0] * 4   # B = 0: nothing to do
    assert f(odd, p, p, null, 0, 1, 8, 5, 8, 8, q, null) == -6       # MTR_E_ALIGN: x, weight, y, residual
    assert f(p, odd, p, null, 0, 1, 8, 5, 8, 8, q, null) == -6
    assert f(p, p, p, null, 0, 1, 8, 5, 8, 8, ctypes.c_void_p(obase + 8), null) == -6
    assert f(p, p, p, odd, 0, 1, 8, 5, 8, 8, q, null) == -6
    assert f(odd, p, p, null, 0, 1, 8, 5, 8, 8, odd, null) == -6     # alignment comes before the overlap
    assert f(p, p, p, null, 0, 1, 8, 5, 8, 8, p, null) == -4         # MTR_E_PARAM: y is x
    assert f(p, p, p, q, 0, 1, 8, 5, 8, 8, q, null) == -4            # y is the residual
    inside = ctypes.c_void_p(base + 256)
    assert f(p, p, p, null, 0, 1, 8, 5, 8, 8, inside, null) == -4    # y overlaps x
    assert f(inside, p, p, p, 0, 1, 8, 5, 8, 8, ctypes.c_void_p(base + 128), null) == -4   # y overlaps the residual
    assert all(v == 0.0 for v in out)


def test_loaders_pass_split3x3_through(tmp_path):
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
    S3 = backbones.SplitConv3x3BiasAct
    m = loading.load_crop_model(d, split3x3=True)   # always the folded copy with fused epilogues
    assert sum(isinstance(k, S3) for k in m.backbone.modules()) == 8
    assert list(m.state_dict()) == list(loading.load_crop_model(d, fold_batchnorm=True, fused_epilogue=True).state_dict())
    m = loading.load_crop_model(d, dtype=torch.float32, split3x3=True, winograd3x3=True)
    mods = [k for k in m.backbone.modules() if isinstance(k, S3)]
    assert len(mods) == 8 and all(k.winograd for k in mods)
    assert not any(isinstance(k, S3) for k in loading.load_crop_model(d).backbone.modules())
    for dtype in (F16, BF16):
        with pytest.raises(ValueError, match='split3x3'):
            loading.load_crop_model(d, dtype=dtype, split3x3=True)
    assert 'split3x3=split3x3' in inspect.getsource(loading.load_multiperson_model)

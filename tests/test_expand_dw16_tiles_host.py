"""CPU: K27h (csrc/expand_dw16_tiles.hip) before it runs on a GPU -- the host-side shape query and refusals of the C
entry on host buffers (a refusal precedes any launch, nothing is read), fold_batchnorm(fuse_expand_depthwise_tiles=True)
on all four backbones (what it arms -- the stride-2 pairs without a folded padding too --, the unchanged state_dict, no
stale reference, beside the other 16-bit options, K25h's and K26h's among them), the loaders' signatures, the code
object's resources, and the armed copy on the CPU, where every layer refuses."""
import ctypes
import inspect

import pytest
import torch

from metrabs_amd import _lib
from test_backbone_option_combos_host import H16_OPTS, NAMES, _net, fold, signature, stale_references, subsets

OK, E_NULL, E_SHAPE, E_DTYPE, E_PARAM, E_ALIGN = 0, -1, -2, -3, -4, -6
F32, F16, BF16 = 0, 1, 2

_store = (ctypes.c_char * (1 << 18))()
_base = (ctypes.addressof(_store) + 255) & ~255
# 16-byte aligned and far enough apart that no tensor of the shapes below overlaps another
X, Y, W1, B1, WD, B2 = (_base + i * 32768 for i in range(6))

NEW = 'fuse_expand_depthwise_tiles'
OTHERS = H16_OPTS + ('fuse_expand_depthwise', 'fuse_expand_depthwise_planes')   # the 16-bit family before the new option
# the pairs fuse_expand_depthwise arms (tests/test_expand_dw16_host.py), and the stride-2 pairs without a folded padding
PAIRS_S1 = {'efficientnetv2-s': 28, 'efficientnetv2-l': 59, 'mobilenetv3': 6, 'resnet18': 0}
PAIRS_S2 = {'efficientnetv2-s': 0, 'efficientnetv2-l': 0, 'mobilenetv3': 2, 'resnet18': 0}


def in_domain(H, W, stride):
    """The plane rule of the entry, restated."""
    from metrabs_amd import kernels
    if not (0 < H <= 128 and 0 < W <= 128):
        return False
    if stride == 1:
        return W % 4 == 0 and W >= 4 and (H * W) % 8 == 0 and not kernels.k11_takes_block_kernel(H, W)
    return stride == 2 and H % 2 == 0 and W % 8 == 0


def _call(lib, x=X, dtype=F16, w1=W1, b1=B1, act1=0, wd=WD, b2=B2, act2=0, B=1, Cin=8, Cmid=8, H=6, W=4, stride=1, y=Y):
    return lib.mtr_expand_dw16_tiles(x, dtype, w1, b1, act1, wd, b2, act2, B, Cin, Cmid, H, W, stride, y, None)


def test_the_shape_query_accepts_exactly_the_domain():
    lib = _lib.load()
    q = lib.mtr_expand_dw16_tiles_lds_bytes
    for Cin, Cmid in [(40, 240), (24, 72), (16, 64)]:
        seen = 0
        for stride in (1, 2):
            for H in range(1, 133):
                for W in range(1, 133):
                    n = q(2, Cin, Cmid, H, W, stride)
                    assert (n > 0) == in_domain(H, W, stride), (H, W, stride)
                    assert n <= 160 * 1024, (H, W, stride)
                    seen += n > 0
        assert seen > 3000
    # MobileNetV3's three classes, and planes K26h takes too (the module-level rule keeps the two apart)
    for H, W, s in [(64, 64, 1), (128, 128, 2), (32, 32, 2), (12, 12, 1), (24, 24, 1), (128, 128, 1), (2, 8, 2)]:
        assert in_domain(H, W, s) and q(1, 8, 8, H, W, s) > 0, (H, W, s)
    # block-kernel planes keep the chain at stride 1 and are taken at stride 2; odd sizes; other strides
    for H, W, s in [(32, 32, 1), (16, 32, 1), (16, 16, 1), (8, 8, 1), (4, 4, 1), (7, 8, 2), (8, 12, 2), (8, 4, 2),
                    (130, 8, 2), (8, 136, 1), (3, 4, 1), (64, 64, 0), (64, 64, 3), (64, 64, -1)]:
        assert not in_domain(H, W, s) and q(1, 8, 8, H, W, s) == 0, (H, W, s)
    assert q(1, 8, 8, 32, 32, 2) > 0 and q(1, 8, 8, 16, 16, 2) > 0
    assert q(1, 12, 8, 64, 64, 1) == 0 and q(1, 8, 0, 64, 64, 1) == 0 and q(1, 0, 8, 64, 64, 1) == 0
    assert q(0, 8, 8, 64, 64, 1) == 0 and q(-1, 8, 8, 64, 64, 1) == 0
    assert q(1 << 27, 8, 8, 12, 12, 1) == 0 and q((1 << 27) - 1, 8, 8, 12, 12, 1) > 0   # B Cmid < 2^30: K11's own limit
    # the entry agrees with the query
    for H, W, s in [(64, 64, 1), (12, 12, 1), (6, 8, 1), (2, 4, 1), (128, 128, 2), (2, 8, 2), (32, 32, 2)]:
        assert _call(lib, B=0, H=H, W=W, stride=s) == OK, (H, W, s)
    for H, W, s in [(8, 8, 1), (32, 32, 1), (3, 4, 1), (7, 8, 2), (8, 12, 2), (132, 8, 2), (64, 64, 3), (64, 64, 0)]:
        assert _call(lib, B=0, H=H, W=W, stride=s) == E_SHAPE and _call(lib, B=1, H=H, W=W, stride=s) == E_SHAPE
    assert _call(lib, Cin=12) == E_SHAPE and _call(lib, Cmid=0) == E_SHAPE and _call(lib, B=-1) == E_SHAPE


def test_unknown_activation_codes_are_refused_before_anything_else_runs():
    """As tests/test_act_code_refusals.py asks of every entry with an `int act` (this one spells its two codes
    act1_code and act2_code): 0 .. 3 with B = 0 are accepted, -1 and 4 are MTR_E_PARAM, on host buffers."""
    lib = _lib.load()
    for which in ('act1', 'act2'):
        for stride, H, W in ((1, 6, 4), (2, 4, 8)):
            assert [_call(lib, B=0, H=H, W=W, stride=stride, **{which: a}) for a in range(4)] == [OK] * 4
            assert _call(lib, H=H, W=W, stride=stride, **{which: -1}) == E_PARAM
            assert _call(lib, H=H, W=W, stride=stride, **{which: 4}) == E_PARAM
            # (the argument checks come before "B == 0")
            assert _call(lib, B=0, H=H, W=W, stride=stride, **{which: 4}) == E_PARAM


def test_null_pointers_dtypes_misalignment_and_overlap_are_refused():
    lib = _lib.load()
    for name in ('x', 'w1', 'b1', 'wd', 'b2', 'y'):
        assert _call(lib, **{name: None}) == E_NULL, name
    assert _call(lib, dtype=F32) == E_DTYPE and _call(lib, dtype=3) == E_DTYPE
    assert _call(lib, B=0, dtype=BF16) == OK
    for name in ('x', 'w1', 'y'):
        assert _call(lib, **{name: globals()[name.upper()] + 8}) == E_ALIGN, name
    for name, base in (('b1', B1), ('wd', WD), ('b2', B2)):
        assert _call(lib, **{name: base + 2}) == E_ALIGN, name
    assert _call(lib, y=X) == E_PARAM and _call(lib, B=0, y=X) == E_PARAM          # y is x
    assert _call(lib, B=2, y=X + 256) == E_PARAM and _call(lib, B=2, x=X + 256, y=X) == E_PARAM   # a partial overlap
    assert _call(lib, B=0, y=X + 256) == OK                                        # (two empty ranges)
    # stride 2: y has a quarter of the positions -- x [2, 8, 4, 8] is 1024 bytes, y [2, 8, 2, 4] is 256
    assert _call(lib, B=2, H=4, W=8, stride=2, x=X + 128, y=X) == E_PARAM
    assert _call(lib, B=0, H=4, W=8, stride=2, x=X + 128, y=X) == OK
    assert _call(lib, B=2, H=4, W=8, stride=2, y=X + 512) == E_PARAM       # (inside x's 1024 bytes)
    assert _call(lib, B=2, H=4, W=8, stride=2, x=X + 248, y=X) == E_ALIGN  # (alignment before overlap)
    # the order: NULL, dtype, shape, parameters, alignment, overlap
    assert _call(lib, x=None, dtype=F32) == E_NULL
    assert _call(lib, dtype=F32, H=8, W=8) == E_DTYPE
    assert _call(lib, H=8, W=8, act1=7) == E_SHAPE and _call(lib, stride=3, act1=7) == E_SHAPE
    assert _call(lib, act2=7, x=X + 8) == E_PARAM
    assert _call(lib, x=X + 16, y=X) == E_PARAM and _call(lib, x=X + 8, y=X) == E_ALIGN


def test_the_option_needs_a_16bit_copy_and_is_off_by_default():
    from metrabs_amd import backbones, loading
    for fn in (backbones.fold_batchnorm, loading.load_crop_model, loading.load_multiperson_model):
        assert inspect.signature(fn).parameters[NEW].default is False, fn.__name__
    net = _net('mobilenetv3')
    with pytest.raises(ValueError, match='fuse_expand_depthwise_tiles=True needs a 16-bit copy'):
        backbones.fold_batchnorm(net, fused_epilogue=True, fuse_expand_depthwise_tiles=True)
    with pytest.raises(ValueError):
        backbones.fold_batchnorm(net, fuse_expand_depthwise_tiles=True)
    with pytest.raises(ValueError, match='load_crop_model: fuse_expand_depthwise_tiles=True needs dtype='):
        loading.load_crop_model('/nonexistent', fuse_expand_depthwise_tiles=True)
    with pytest.raises(ValueError, match='fuse_expand_depthwise_tiles=True needs dtype='):
        loading.load_multiperson_model('/nonexistent', fuse_expand_depthwise_tiles=True)
    assert (NEW, '16bit') in backbones._OPTION_NEEDS
    assert [o for o, _ in backbones._OPTION_NEEDS].count(NEW) == 1
    D = backbones.DepthwiseBiasAct
    assert D.use_k27h is True and isinstance(D.k27h_slower, frozenset)
    assert all(len(key) == 5 and key[4] in (1, 2) for key in D.k27h_slower)
    assert backbones.ConvBiasAct.hand_tiles_to == ()


def _armed(copy, field):
    from metrabs_amd import backbones
    return [(n, m, getattr(m, field)[0]) for n, m in copy.named_modules()
            if isinstance(m, backbones.ConvBiasAct) and getattr(m, field)]


@pytest.mark.parametrize('name', NAMES)
def test_the_armed_pairs_are_those_of_fuse_expand_depthwise_and_the_plain_stride_2_pairs(name):
    from metrabs_amd import backbones
    plain = fold(_net(name), torch.bfloat16, ())
    armed = fold(_net(name), torch.bfloat16, (NEW,))
    k25h = fold(_net(name), torch.bfloat16, ('fuse_expand_depthwise',))
    k26h = fold(_net(name), torch.bfloat16, ('fuse_expand_depthwise_planes',))
    # hand_to and hand_planes_to are armed only by their own options, hand_tiles_to only by the new one
    assert not _armed(plain, 'hand_tiles_to') and not _armed(k25h, 'hand_tiles_to') and not _armed(k26h, 'hand_tiles_to')
    assert not any('hand_tiles_to' in m.__dict__ for m in plain.modules())
    assert not _armed(armed, 'hand_to') and not _armed(armed, 'hand_planes_to')
    assert not _armed(k25h, 'hand_planes_to') and not _armed(k26h, 'hand_to')
    assert len(_armed(k25h, 'hand_to')) == PAIRS_S1[name] == len(_armed(k26h, 'hand_planes_to'))
    assert list(armed.state_dict()) == list(plain.state_dict())
    assert [(n, type(m)) for n, m in armed.named_modules()] == [(n, type(m)) for n, m in plain.named_modules()]
    assert [n for n, _ in armed.named_buffers()] == [n for n, _ in plain.named_buffers()]
    pairs = _armed(armed, 'hand_tiles_to')
    s1 = [(n, e, d) for n, e, d in pairs if d.stride == 1]
    s2 = [(n, e, d) for n, e, d in pairs if d.stride == 2]
    assert len(s1) == PAIRS_S1[name] and len(s2) == PAIRS_S2[name] and len(pairs) == len(s1) + len(s2)
    assert [n for n, _, _ in s1] == [n for n, _, _ in _armed(k25h, 'hand_to')]
    mods = dict(armed.named_modules())
    for n, e, d in pairs:
        assert n.endswith('.block.0.0') and mods[n[:-len('0.0')] + '1.0'] is d, n
        assert type(e) is backbones.ConvBiasAct and isinstance(d, backbones.DepthwiseBiasAct)
        assert (d.k, d.pad, d.pads) == (3, 1, None) and not e.emit_mean
        assert d.weight.shape[0] == e.conv.out_channels
    if name == 'mobilenetv3':
        assert sorted((e.conv.in_channels, e.conv.out_channels) for _, e, _ in s2) == [(16, 64), (40, 240)]
    # every other stride-2 depthwise 3x3 layer carries a folded padding or feeds a squeeze-excite block (EfficientNetV2's
    # one symmetric stride-2 block), which K27h, having no mean, cannot serve
    armed_dw = {id(d) for _, _, d in pairs}
    for m in armed.modules():
        if isinstance(m, backbones.DepthwiseBiasAct) and m.stride == 2 and m.k == 3 and id(m) not in armed_dw:
            assert m.pads is not None or m.emit_mean, name


@pytest.mark.parametrize('name', NAMES)
def test_no_stale_reference_beside_the_other_16bit_options(name):
    """Every subset of the six other 16-bit options (fuse_expand_depthwise and fuse_expand_depthwise_planes among them)
    together with the new one: no reference to a module outside the tree, the default copy's keys, and no field armed
    twice -- the new option changes hand_tiles_to of the expands and nothing that signature() sees."""
    from metrabs_amd import backbones
    keys = list(fold(_net(name), torch.bfloat16, ()).state_dict())
    n_pairs = PAIRS_S1[name] + PAIRS_S2[name]
    assert len(subsets(OTHERS)) == 64
    for s in subsets(OTHERS):
        opts = tuple(sorted(s)) + (NEW,)
        copy = fold(_net(name), torch.bfloat16, opts)
        mods = {id(m) for m in copy.modules()}
        assert stale_references(copy) == [], opts
        pairs = _armed(copy, 'hand_tiles_to')
        assert len(pairs) == n_pairs, opts
        assert all(id(d) in mods and isinstance(d, backbones.DepthwiseBiasAct) for _, _, d in pairs), opts
        for field in ('hand_planes_to', 'hand_to'):   # (hand_to: the stem's Preproc too, which stale_references covers)
            assert all(id(d) in mods for _, _, d in _armed(copy, field)), (opts, field)
        assert list(copy.state_dict()) == keys, opts
        assert len(_armed(copy, 'hand_to')) == (PAIRS_S1[name] if 'fuse_expand_depthwise' in s else 0), opts
        assert len(_armed(copy, 'hand_planes_to')) == (PAIRS_S1[name] if 'fuse_expand_depthwise_planes' in s else 0), opts
        assert signature(copy) == signature(fold(_net(name), torch.bfloat16, tuple(sorted(s)))), opts


@pytest.mark.parametrize('name', NAMES)
def test_the_armed_copy_on_the_cpu_is_the_default_copy(name):
    plain, armed = fold(_net(name), torch.bfloat16, ()), fold(_net(name), torch.bfloat16, OTHERS + (NEW,))
    x = torch.rand(2, 3, 96, 96, generator=torch.Generator().manual_seed(2))
    with torch.inference_mode():
        a, p = armed(x), plain(x)
    assert a.dtype == torch.bfloat16 and torch.isfinite(a.float()).all()
    assert torch.equal(a, p)
    paths = {getattr(m, 'last_path', None) for m in armed.modules()}
    assert paths <= {None, 'library', 'chain'}, paths
    only = fold(_net(name), torch.bfloat16, (NEW,))
    with torch.inference_mode():
        assert torch.equal(only(x), p)
    assert [getattr(m, 'last_path', None) for m in only.modules()] == [getattr(m, 'last_path', None)
                                                                       for m in plain.modules()]


def test_the_kernels_use_no_scratch_and_stay_under_the_lds_limit():
    """tests/test_kernel_resources.py walks every source of the library, this one included; here the new file's own
    instantiations (two dtypes, two strides, two tile counts) by name: no scratch, no spilled VGPR, no static LDS."""
    from metrabs_amd import build
    assert 'expand_dw16_tiles.hip' in build.sources()
    ks = [k for k in build.kernel_resources('expand_dw16_tiles.hip') if 'expand_dw16_tiles_kernel' in k['name']]
    assert len(ks) == 8
    for k in ks:
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, k
        assert k['group_segment_fixed_size'] == 0, k   # (all of its LDS is dynamic: the query's answer)
        assert k['vgpr_count'] + 0 <= 512, k

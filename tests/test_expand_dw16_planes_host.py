"""CPU: K26h (csrc/expand_dw16_planes.hip) before it runs on a GPU -- the host-side shape query and refusals of the C
entry on host buffers (a refusal precedes any launch, nothing is read), fold_batchnorm(fuse_expand_depthwise_planes=True)
on all four backbones (what it arms, the unchanged state_dict, no stale reference, beside the other 16-bit options,
K25h's among them), the loaders' signatures, and the armed copy on the CPU, where every layer refuses."""
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
X, Y, W1, B1, WD, B2, MEAN = (_base + i * 32768 for i in range(7))

NEW = 'fuse_expand_depthwise_planes'
OTHERS = H16_OPTS + ('fuse_expand_depthwise',)   # the 16-bit family before the new option
# the same pairs fuse_expand_depthwise arms (tests/test_expand_dw16_host.py)
PAIRS = {'efficientnetv2-s': 28, 'efficientnetv2-l': 59, 'mobilenetv3': 6, 'resnet18': 0}


def in_domain(H, W):
    """The plane rule of the entry, restated."""
    from metrabs_amd import kernels
    return (H > 0 and W > 0 and W % 4 == 0 and (H * W) % 8 == 0 and H <= 32 and W <= 32 and H * W <= 576
            and not kernels.k11_takes_block_kernel(H, W))


def _call(lib, x=X, dtype=F16, w1=W1, b1=B1, act1=0, wd=WD, b2=B2, act2=0, B=1, Cin=8, Cmid=8, H=6, W=4, y=Y,
          mean=None, mapping=None):
    args = (x, dtype, w1, b1, act1, wd, b2, act2, B, Cin, Cmid, H, W, y, mean, None)
    return lib.mtr_expand_dw16_planes(*args) if mapping is None else lib.mtr_expand_dw16_planes_opts(*args, mapping)


def test_the_shape_query_accepts_exactly_the_domain():
    lib = _lib.load()
    q = lib.mtr_expand_dw16_planes_lds_bytes
    for H, W in [(12, 12), (24, 24), (20, 20), (6, 8), (2, 4), (10, 4), (12, 24), (24, 12), (28, 20), (18, 32)]:
        assert in_domain(H, W) and 0 < q(1, 8, 8, H, W) <= 160 * 1024, (H, W)
    # K25h's planes, the other block-kernel planes, 32x32 and larger, odd rows of positions
    for H, W in [(8, 8), (16, 16), (4, 4), (32, 16), (16, 32), (32, 8), (32, 32), (24, 28), (36, 12), (12, 36), (3, 4),
                 (12, 10), (64, 64)]:
        assert not in_domain(H, W) and q(1, 8, 8, H, W) == 0, (H, W)
    assert q(1, 12, 8, 12, 12) == 0 and q(1, 8, 0, 12, 12) == 0 and q(1, 0, 8, 12, 12) == 0
    assert q(0, 8, 8, 12, 12) == 0 and q(-1, 8, 8, 12, 12) == 0
    assert q(1 << 27, 8, 8, 12, 12) == 0 and q((1 << 27) - 1, 8, 8, 12, 12) > 0   # B Cmid < 2^30: K11's own limit
    seen = 0
    for H in range(1, 41):
        for W in range(1, 41):
            n = q(2, 16, 24, H, W)
            assert (n > 0) == in_domain(H, W), (H, W)
            assert n <= 160 * 1024, (H, W)
            seen += n > 0
    assert seen > 60
    # the entry agrees with the query
    for H, W in [(12, 12), (24, 24), (6, 8), (2, 4)]:
        assert _call(lib, B=0, H=H, W=W) == OK
    for H, W in [(8, 8), (16, 16), (32, 16), (32, 32), (3, 4)]:
        assert _call(lib, B=0, H=H, W=W) == E_SHAPE and _call(lib, B=1, H=H, W=W) == E_SHAPE
    assert _call(lib, Cin=12) == E_SHAPE and _call(lib, Cmid=0) == E_SHAPE and _call(lib, B=-1) == E_SHAPE


def test_unknown_activation_codes_are_refused_before_anything_else_runs():
    """As tests/test_act_code_refusals.py asks of every entry with an `int act` (this one spells its two codes
    act1_code and act2_code): 0 .. 3 with B = 0 are accepted, -1 and 4 are MTR_E_PARAM, on host buffers."""
    lib = _lib.load()
    for which in ('act1', 'act2'):
        assert [_call(lib, B=0, **{which: a}) for a in range(4)] == [OK] * 4
        assert _call(lib, **{which: -1}) == E_PARAM and _call(lib, **{which: 4}) == E_PARAM
        assert _call(lib, B=0, **{which: 4}) == E_PARAM   # (the argument checks come before "B == 0")
    assert [_call(lib, B=0, mapping=m) for m in (-1, 0, 1)] == [OK] * 3
    assert _call(lib, mapping=2) == E_PARAM and _call(lib, mapping=-2) == E_PARAM


def test_null_pointers_dtypes_misalignment_and_overlap_are_refused():
    lib = _lib.load()
    for name in ('x', 'w1', 'b1', 'wd', 'b2', 'y'):
        assert _call(lib, **{name: None}) == E_NULL, name
    assert _call(lib, B=0, mean=None) == OK and _call(lib, B=0, mean=MEAN) == OK   # the mean is optional
    assert _call(lib, dtype=F32) == E_DTYPE and _call(lib, dtype=3) == E_DTYPE
    assert _call(lib, B=0, dtype=BF16) == OK
    for name in ('x', 'w1', 'y'):
        assert _call(lib, **{name: globals()[name.upper()] + 8}) == E_ALIGN, name
    for name, base in (('b1', B1), ('wd', WD), ('b2', B2), ('mean', MEAN)):
        assert _call(lib, **{name: base + 2}) == E_ALIGN, name
    assert _call(lib, y=X) == E_PARAM and _call(lib, B=0, y=X) == E_PARAM          # y is x
    assert _call(lib, B=2, y=X + 256) == E_PARAM and _call(lib, B=2, x=X + 256, y=X) == E_PARAM   # a partial overlap
    assert _call(lib, B=0, y=X + 256) == OK                                        # (two empty ranges)
    # the order: NULL, dtype, shape, parameters, alignment, overlap
    assert _call(lib, x=None, dtype=F32) == E_NULL
    assert _call(lib, dtype=F32, H=8, W=8) == E_DTYPE
    assert _call(lib, H=8, W=8, act1=7) == E_SHAPE
    assert _call(lib, act2=7, x=X + 8) == E_PARAM
    assert _call(lib, x=X + 16, y=X) == E_PARAM and _call(lib, x=X + 8, y=X) == E_ALIGN


def test_the_option_needs_a_16bit_copy_and_is_off_by_default():
    from metrabs_amd import backbones, loading
    for fn in (backbones.fold_batchnorm, loading.load_crop_model, loading.load_multiperson_model):
        assert inspect.signature(fn).parameters[NEW].default is False, fn.__name__
    net = _net('efficientnetv2-s')
    with pytest.raises(ValueError, match='fuse_expand_depthwise_planes=True needs a 16-bit copy'):
        backbones.fold_batchnorm(net, fused_epilogue=True, fuse_expand_depthwise_planes=True)
    with pytest.raises(ValueError):
        backbones.fold_batchnorm(net, fuse_expand_depthwise_planes=True)
    with pytest.raises(ValueError, match='load_crop_model: fuse_expand_depthwise_planes=True needs dtype='):
        loading.load_crop_model('/nonexistent', fuse_expand_depthwise_planes=True)
    with pytest.raises(ValueError, match='fuse_expand_depthwise_planes=True needs dtype='):
        loading.load_multiperson_model('/nonexistent', fuse_expand_depthwise_planes=True)
    assert (NEW, '16bit') in backbones._OPTION_NEEDS
    D = backbones.DepthwiseBiasAct
    assert D.use_k26h is True and isinstance(D.k26h_slower, frozenset)


def _armed(copy, field):
    from metrabs_amd import backbones
    return [(n, m, getattr(m, field)[0]) for n, m in copy.named_modules()
            if isinstance(m, backbones.ConvBiasAct) and getattr(m, field)]


@pytest.mark.parametrize('name', NAMES)
def test_the_armed_pairs_are_those_of_fuse_expand_depthwise(name):
    from metrabs_amd import backbones
    plain = fold(_net(name), torch.bfloat16, ())
    armed = fold(_net(name), torch.bfloat16, (NEW,))
    k25h = fold(_net(name), torch.bfloat16, ('fuse_expand_depthwise',))
    assert not _armed(plain, 'hand_planes_to') and not _armed(k25h, 'hand_planes_to')
    assert not any('hand_planes_to' in m.__dict__ for m in plain.modules())
    assert not _armed(armed, 'hand_to')   # a field of its own
    assert list(armed.state_dict()) == list(plain.state_dict())
    assert [(n, type(m)) for n, m in armed.named_modules()] == [(n, type(m)) for n, m in plain.named_modules()]
    assert [n for n, _ in armed.named_buffers()] == [n for n, _ in plain.named_buffers()]
    pairs = _armed(armed, 'hand_planes_to')
    assert len(pairs) == PAIRS[name]
    assert [n for n, _, _ in pairs] == [n for n, _, _ in _armed(k25h, 'hand_to')]
    mods = dict(armed.named_modules())
    for n, e, d in pairs:
        assert n.endswith('.block.0.0') and mods[n[:-len('0.0')] + '1.0'] is d, n
        assert type(e) is backbones.ConvBiasAct and isinstance(d, backbones.DepthwiseBiasAct)
        assert (d.k, d.stride, d.pad, d.pads) == (3, 1, 1, None)


@pytest.mark.parametrize('name', NAMES)
def test_no_stale_reference_beside_the_other_16bit_options(name):
    """Every subset of the 16-bit options (fuse_expand_depthwise among them) together with the new one: no reference to
    a module outside the tree, the default copy's keys, and no field armed twice -- the new option changes
    hand_planes_to of the expands and nothing that signature() sees."""
    from metrabs_amd import backbones
    keys = list(fold(_net(name), torch.bfloat16, ()).state_dict())
    for s in subsets(OTHERS):
        opts = tuple(sorted(s)) + (NEW,)
        copy = fold(_net(name), torch.bfloat16, opts)
        mods = {id(m) for m in copy.modules()}
        assert stale_references(copy) == [], opts
        pairs = _armed(copy, 'hand_planes_to')
        assert len(pairs) == PAIRS[name], opts
        assert all(id(d) in mods and isinstance(d, backbones.DepthwiseBiasAct) for _, _, d in pairs), opts
        assert list(copy.state_dict()) == keys, opts
        assert len(_armed(copy, 'hand_to')) == (PAIRS[name] if 'fuse_expand_depthwise' in s else 0), opts
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

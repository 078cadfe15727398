"""CPU: fold_batchnorm with several opt-in kernels armed in one copy.  Every subset of the four options of each family
(f32: fuse_stem, block_depthwise, winograd3x3, split_gemm; 16-bit: fuse_blocks, fuse_stem, block_depthwise,
deep_projects), on all four backbones: unchanged state_dict keys, no reference to a module that a later replacement took
out of the tree, arming that composes from the single-option copies, and the all-on copy on the CPU, where no kernel
takes anything.  (tests/test_gpu_backbone_option_combos.py runs the combined copies on the GPU and uses the helpers
below.)"""
import collections
import functools
import itertools

import pytest
import torch

NAMES = ['efficientnetv2-s', 'efficientnetv2-l', 'mobilenetv3', 'resnet18']
F32_OPTS = ('fuse_stem', 'block_depthwise', 'winograd3x3', 'split_gemm')
H16_OPTS = ('fuse_blocks', 'fuse_stem', 'block_depthwise', 'deep_projects')
FAMILIES = {'f32': (None, F32_OPTS), '16bit': (torch.bfloat16, H16_OPTS)}

# attributes that hold references to other modules of the same copy (never registered submodules)
REFERENCES = ('mean_from', 'gate_to', 'pre_pair', 'fused_pair', 'hand_to')
FIELDS = ('cls', 'split_gemm', 'block_depthwise', 'deep_projects', 'pre_pair', 'fused_pair', 'hand_to', 'mean_from',
          'gate_to')


def subsets(opts):
    return [frozenset(c) for n in range(len(opts) + 1) for c in itertools.combinations(opts, n)]


def fold(net, dtype, opts):
    from metrabs_amd import backbones
    return backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, **{o: True for o in opts})


def signature(copy):
    """{module name: {field: value}}: what the options arm, per module."""
    sig = collections.OrderedDict()
    for name, m in copy.named_modules():
        sig[name] = dict(
            cls=type(m).__name__,
            split_gemm=bool(getattr(m, 'split_gemm', False)),
            block_depthwise=bool(getattr(m, 'block_depthwise', False)),
            deep_projects=bool(getattr(m, 'deep_projects', False)),
            pre_pair=tuple(type(k).__name__ for k in getattr(m, 'pre_pair', ())),
            fused_pair=tuple(type(k).__name__ for k in getattr(m, 'fused_pair', ())),
            hand_to=len(getattr(m, 'hand_to', ())),
            mean_from=len(getattr(m, 'mean_from', ())),
            gate_to=len(getattr(m, 'gate_to', ())))
    return sig


def stale_references(copy):
    """[(module name, attribute, class of the referenced object)] for every reference to an object that is no module of
    `copy` any more, or that stands at another place than the attribute promises."""
    mods = {id(m) for m in copy.modules()}
    bad = []
    for name, m in copy.named_modules():
        for attr in REFERENCES:
            for obj in getattr(m, attr, ()):
                if id(obj) not in mods:
                    bad.append((name, attr, type(obj).__name__))
        for attr in ('pre_pair', 'fused_pair'):   # (the block's own two layers, by identity)
            pair = getattr(m, attr, ())
            if pair and not (pair[0] is m.block._modules['0'][0] and pair[1] is m.block._modules['1'][0]):
                bad.append((name, attr, 'not the layers of this block'))
    return bad


def changed_by(default, singles, prefix=None):
    """{(module name, field): [the options whose single-option copy differs from the default copy there]}, for the
    modules at or below `prefix` (all of them: None)."""
    out = {}
    for name, fields in default.items():
        if prefix is not None and name != prefix and not name.startswith(prefix + '.'):
            continue
        for f in FIELDS:
            who = [o for o, sig in singles.items() if sig[name][f] != fields[f]]
            if who:
                out[(name, f)] = who
    return out


# Where two options change the same field of the same module, the expected value is written down here, not derived:
# {(family, field, the default copy's value, frozenset of the options): the value with all of them on}.  No such place
# exists today -- the stem is stride 2 (K19 wants stride 1), has 3 input channels (K14h wants a multiple of 8) and is no
# 1x1 layer, and every other option arms another class of layer -- so the table is empty, and a new overlap fails the
# test until its outcome is stated here.
OVERLAPS = {}


@functools.lru_cache(maxsize=None)
def _net(name):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    return backbones.build_backbone(name).eval()


@functools.lru_cache(maxsize=None)
def _survey(name, family):
    """Folds all 16 copies of one family once and keeps only what the assertions need (the copies themselves go)."""
    dtype, opts = FAMILIES[family]
    out = {}
    for s in subsets(opts):
        copy = fold(_net(name), dtype, s)
        out[s] = dict(keys=list(copy.state_dict()), sig=signature(copy), stale=stale_references(copy))
    return out


CASES = [(n, f) for n in NAMES for f in FAMILIES]


@pytest.mark.parametrize('name,family', CASES)
def test_state_dict_keys_are_the_default_copys(name, family):
    survey = _survey(name, family)
    assert len(survey) == 16
    want = survey[frozenset()]['keys']
    for s, got in survey.items():
        assert got['keys'] == want, sorted(s)


@pytest.mark.parametrize('name,family', CASES)
def test_no_reference_to_a_replaced_module(name, family):
    """mean_from, gate_to, pre_pair, fused_pair and hand_to are taken at different moments of fold_batchnorm, between
    which modules are replaced by new objects (WinogradConv3x3BiasAct, Conv3x3BiasAct, StemConvBiasAct): every object
    they hold must still be a module of the copy.  (Seen to fail with the winograd3x3 replacement moved below the
    pre_pair wiring: 6 stale pre_pair[0] per EfficientNetV2-S copy with that option.)"""
    survey = _survey(name, family)
    n_refs = 0
    for s, got in survey.items():
        assert got['stale'] == [], (sorted(s), got['stale'][:4])
        n_refs += sum(len(v[a]) if isinstance(v[a], tuple) else v[a] for v in got['sig'].values()
                      for a in REFERENCES)
    if name != 'resnet18':     # (ResNet-18 has no squeeze-excite block, FusedMBConv or Preproc: nothing to hold)
        assert n_refs > 0


@pytest.mark.parametrize('name,family', CASES)
def test_arming_composes_from_the_single_option_copies(name, family):
    _, opts = FAMILIES[family]
    survey = _survey(name, family)
    default = survey[frozenset()]['sig']
    singles = {o: survey[frozenset([o])]['sig'] for o in opts}
    for sig in singles.values():
        assert list(sig) == list(default)            # the same module tree, name by name
    changed = changed_by(default, singles)
    for s, got in survey.items():
        sig = got['sig']
        assert list(sig) == list(default), sorted(s)
        for mod, fields in sig.items():
            for f in FIELDS:
                who = [o for o in changed.get((mod, f), ()) if o in s]
                if not who:
                    want = default[mod][f]
                elif len(who) == 1:
                    want = singles[who[0]][mod][f]
                else:
                    key = (family, f, default[mod][f], frozenset(who))
                    assert key in OVERLAPS, ('two options change one field: state the outcome in OVERLAPS', mod, key)
                    want = OVERLAPS[key]
                assert fields[f] == want, (sorted(s), mod, f, fields[f], want)


# what the options arm, stated from the architecture tables (not from the code under test):
# (FusedMBConv blocks with an expand and a project, of which stride 1; dense 3x3 stride-1 Cin % 4 == 0 layers;
#  depthwise 3x3 stride-1 layers without folded padding; deep projects Cin >= 768, Cout > 160; 3x3 s2 Cin = 3 stem)
ARCH = {
    'efficientnetv2-s': dict(pairs=8, pairs_s1=6, wino=8, dw=28, deep=15, stem=1),
    'efficientnetv2-l': dict(pairs=14, pairs_s1=12, wino=16, dw=59, deep=60, stem=1),
    'mobilenetv3': dict(pairs=0, pairs_s1=0, wino=0, dw=7, deep=0, stem=1),
    'resnet18': dict(pairs=0, pairs_s1=0, wino=13, dw=0, deep=0, stem=0),
}


@pytest.mark.parametrize('name,family', CASES)
def test_the_all_on_copy_arms_what_the_architecture_says(name, family):
    """The fields that a second option could plausibly disturb, counted in the all-on copy against numbers taken from the
    architecture tables: pre_pair[0]'s class under winograd3x3 (WinogradConv3x3BiasAct on the stride-1 blocks, the plain
    ConvBiasAct on the stride-2 ones), pre_pair[1] armed for K20, fused_pair beside deep_projects, the stem beside
    everything."""
    _, opts = FAMILIES[family]
    a = ARCH[name]
    sig = _survey(name, family)[frozenset(opts)]['sig']
    count = lambda pred: sum(bool(pred(v)) for v in sig.values())
    assert count(lambda v: v['cls'] == 'StemConvBiasAct') == a['stem'] == count(lambda v: v['hand_to'] == 1)
    assert count(lambda v: v['block_depthwise']) == a['dw']
    if family == 'f32':
        assert count(lambda v: v['pre_pair'] == ('WinogradConv3x3BiasAct', 'ConvBiasAct')) == a['pairs_s1']
        assert count(lambda v: v['pre_pair'] == ('ConvBiasAct', 'ConvBiasAct')) == a['pairs'] - a['pairs_s1']
        assert count(lambda v: v['cls'] == 'WinogradConv3x3BiasAct') == a['wino']
        assert count(lambda v: v['fused_pair']) == 0 and count(lambda v: v['deep_projects']) == 0
        # every project behind a pre_pair is armed for K20, and no 3x3 layer is
        for mod, v in sig.items():
            if v['pre_pair']:
                assert sig[mod + '.block.1.0']['split_gemm'] and not sig[mod + '.block.0.0']['split_gemm'], mod
    else:
        assert count(lambda v: v['fused_pair'] == ('Conv3x3BiasAct', 'ConvBiasAct')) == a['pairs']
        assert count(lambda v: v['deep_projects']) == a['deep']
        assert count(lambda v: v['pre_pair']) == 0 and count(lambda v: v['split_gemm']) == 0
        assert count(lambda v: v['cls'] == 'WinogradConv3x3BiasAct') == 0


@pytest.mark.parametrize('name,family', CASES)
def test_the_all_on_copy_on_the_cpu_is_the_default_copy(name, family):
    dtype, opts = FAMILIES[family]
    plain, armed = fold(_net(name), dtype, ()), fold(_net(name), dtype, opts)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    with torch.inference_mode():
        a, p = armed(x), plain(x)
    assert a.dtype == (dtype or torch.float32) and torch.isfinite(a.float()).all()
    assert torch.equal(a, p)
    paths = {getattr(m, 'last_path', None) for m in armed.modules()}
    assert paths <= {None, 'library', 'chain'}, paths
    assert 'library' in paths

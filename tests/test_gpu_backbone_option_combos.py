"""GPU: folded backbone copies with several opt-in kernels armed at once (fold_batchnorm's fuse_stem, block_depthwise,
winograd3x3, split_gemm on an f32 copy; fuse_blocks, fuse_stem, block_depthwise, deep_projects on a 16-bit copy).  Each
option has its own tests; here they run together: every option's kernel runs inside an all-on copy, every unit of the
all-on copy returns the bits (and takes the paths) of a copy armed with that unit's options alone, the class switches
take the all-on copy back to the single-option copies bit for bit, the all-on copies meet the accuracy criteria of the
single options, and they work through the loader and the API."""
import contextlib
import copy
import functools

import pytest
import torch

from oracle import cases
from test_backbone_option_combos_host import F32_OPTS, H16_OPTS, changed_by, fold, signature
from test_gpu_conv1x1_split import _Fp64Backbone, _all_paths, _model_dir, _pinned

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
DEEP = ('k13h_deep', 'k13h_deep_gate')
FAMILY_OPTS = {None: F32_OPTS, F16: H16_OPTS, BF16: H16_OPTS}
# (network, crop side, batch).  EfficientNetV2-S at 256 px: K19, K16h, the deep projects on 8x8 maps.  At 192 px: 12x12
# planes for K18, and 6x6 maps, where the deep-K and the other 1x1 kernels refuse inside an armed copy.  MobileNetV3 at
# 256 px: K18 on 128x128 and 64x64 planes.  K17 and K20 run in all three.
SETS = [('efficientnetv2-s', 256, 2), ('efficientnetv2-s', 192, 2), ('mobilenetv3', 256, 1)]


@functools.lru_cache(maxsize=None)
def _calibrated(name):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    return backbones.calibrate_batchnorm(backbones.build_backbone(name).cuda(), 256, 'cuda', batch_size=4)


@functools.lru_cache(maxsize=None)
def _copy(name, dtype, opts):
    """The folded copy of the calibrated `name` with exactly `opts` (a frozenset) on: made once, shared, never written."""
    return fold(_calibrated(name), dtype, opts)


def _input(res, batch, seed=1):
    return torch.rand(batch, 3, res, res, device='cuda', generator=torch.Generator(device='cuda').manual_seed(seed))


def _reset_paths(*mods):
    """The copies are shared between tests: whatever an earlier forward left in .last_path goes."""
    for top in mods:
        for m in top.modules():
            if hasattr(m, 'last_path'):
                m.last_path = None


def _forward(net, x):
    _reset_paths(net)
    with torch.inference_mode(), _pinned():
        y = net(x).clone()
    return y, _all_paths(net)


def _switch_table():
    from metrabs_amd import backbones as B
    return {'fuse_stem': (B.StemConvBiasAct, 'use_k17'), 'block_depthwise': (B.DepthwiseBiasAct, 'use_k18'),
            'winograd3x3': (B.WinogradConv3x3BiasAct, 'use_k19'), 'split_gemm': (B.ConvBiasAct, 'use_k20'),
            'fuse_blocks': (B.FusedMBConv, 'use_k16h')}


@contextlib.contextmanager
def _switched_off(opts):
    table = _switch_table()
    saved = [(cls, attr, cls.__dict__[attr]) for cls, attr in (table[o] for o in opts)]
    try:
        for cls, attr, _ in saved:
            setattr(cls, attr, False)
        yield
    finally:
        for cls, attr, was in saved:
            setattr(cls, attr, was)


# ---- every option's kernel runs inside a copy that has all of them on

@pytest.mark.parametrize('dtype', [None, F16, BF16])
def test_every_opt_in_kernel_runs_inside_an_all_on_copy(dtype, hip_lib):
    from metrabs_amd import backbones
    seen = {}
    for name, res, batch in SETS:
        net = _copy(name, dtype, frozenset(FAMILY_OPTS[dtype]))
        y, paths = _forward(net, _input(res, batch))
        assert torch.isfinite(y).all() and y.dtype == (dtype or torch.float32)
        seen[(name, res)] = set(paths)
        if dtype is not None and (name, res) == ('efficientnetv2-s', 192):
            # 6x6 maps: the armed deep projects fall back to the library path inside the armed copy
            deep = [m.last_path for m in net.modules() if isinstance(m, backbones.ConvBiasAct) and m.deep_projects]
            assert len(deep) == 15 and set(deep) == {'library'}, deep
        if dtype is None and (name, res) == ('efficientnetv2-s', 256):
            # a block on its 'k19' branch: the 3x3 layer with its own epilogue on K19, then the project on K20
            k19 = [m for m in net.modules() if isinstance(m, backbones.FusedMBConv) and m.last_path == 'k19']
            assert len(k19) == 6 and {m.pre_pair[0].last_path for m in k19} == {'k19'}
            assert {m.pre_pair[1].last_path for m in k19} == {'k20'}
    union = set().union(*seen.values())
    if dtype is None:
        assert {'k17', 'k18', 'k19', 'k20', 'k20_gate', 'k20_pre'} <= union, seen
        assert 'k19' in seen[('efficientnetv2-s', 256)] and 'k18' in seen[('efficientnetv2-s', 192)]
        assert {'k17', 'k18', 'k20', 'k20_gate'} <= seen[('mobilenetv3', 256)], seen
    else:
        assert {'k16h', 'k17', 'k18'} <= union and union & set(DEEP), seen
        assert {'k16h', 'k17'} <= seen[('efficientnetv2-s', 256)] and seen[('efficientnetv2-s', 256)] & set(DEEP)
        assert 'k18' in seen[('efficientnetv2-s', 192)] and {'k17', 'k18'} <= seen[('mobilenetv3', 256)], seen


@pytest.mark.parametrize('dtype', [None, F16])
def test_derived_weight_caches_of_an_all_on_copy_hold_the_present_weights(dtype, hip_lib):
    """weight_split() (K20), weight_u() (K19) and _fc2_wt() (K12) are keyed by the weight's pointer and version, and
    live on modules that other options replace or cast: after a forward each holds what a fresh transform of the
    weight the module has now gives."""
    from metrabs_amd import backbones, kernels
    net = _copy('efficientnetv2-s', dtype, frozenset(FAMILY_OPTS[dtype]))
    _forward(net, _input(256, 2))
    n = dict(ws=0, wu=0, w2t=0)
    for m in net.modules():
        if getattr(m, '_ws', None) is not None:
            n['ws'] += 1
            assert torch.equal(m._ws[1], kernels.pack_conv1x1_split_weight(m.conv.weight))
        if getattr(m, '_wu', None) is not None:
            n['wu'] += 1
            assert torch.equal(m._wu[1], kernels.pack_conv3x3_winograd_weight(m.conv.weight))
        if isinstance(m, backbones.SqueezeExcite) and m._w2t is not None:
            n['w2t'] += 1
            w = m.fc2.weight
            assert m._w2t[1].dtype == torch.float32 and torch.equal(m._w2t[1], w.reshape(w.shape[0], -1).t())
    assert n['w2t'] == 30 and (n['ws'] > 30 and n['wu'] == 8 if dtype is None else n['ws'] == n['wu'] == 0), n


# ---- A: every unit of the all-on copy against the copy armed with that unit's options alone

def _units(net):
    """[[module name, ...]]: the module(s) of each unit in running order -- the stem pair (Preproc and the first
    ConvBNAct), every block, every other ConvBNAct outside the blocks."""
    from metrabs_amd import backbones as B
    named = list(net.named_modules())
    blocks = [n for n, m in named if isinstance(m, (B.MBConv, B.FusedMBConv, B.MBv3Block, B.BasicBlock))]
    inside = lambda n: any(n.startswith(b + '.') for b in blocks)
    convs = [n for n, m in named if isinstance(m, B.ConvBNAct) and not inside(n)]
    pre = [n for n, m in named if isinstance(m, B.Preproc)]
    assert len(pre) == 1 and len(convs) >= 2 and len(blocks) >= 15
    return [[pre[0], convs[0]]] + [[n] for n in blocks] + [[n] for n in convs[1:]]


def _unit_paths(mods):
    return [getattr(k, 'last_path', None) for m in mods for k in m.modules()]


def _record(net, units, x):
    """One forward of `net`: {unit: (its input, its output, the last_path list of its modules)}, copies all."""
    rec, hooks = {}, []
    for names in units:
        mods = [net.get_submodule(n) for n in names]
        key = tuple(names)
        hooks.append(mods[0].register_forward_pre_hook(
            lambda mod, args, key=key: rec.__setitem__(key, [args[0].clone()])))
        hooks.append(mods[-1].register_forward_hook(
            lambda mod, args, out, key=key, mods=mods: rec[key].extend([out.clone(), _unit_paths(mods)])))
    try:
        _reset_paths(net)
        with torch.inference_mode(), _pinned():
            net(x)
    finally:
        for h in hooks:
            h.remove()
    return rec


@pytest.mark.parametrize('dtype', [None, F16, BF16])
@pytest.mark.parametrize('name,res,batch', SETS)
def test_units_of_the_all_on_copy_replay_exactly(name, res, batch, dtype, hip_lib):
    """A unit receives one tensor and hands one on: no gate, mean or hand-over crosses its border, so each unit is a
    deterministic function of its input and of the options that arm something inside it.  The all-on copy's unit must
    return, on the input it saw, the bits of the same unit in the copy folded with those options alone, on the same
    paths.  Anything else is interference between options."""
    opts = FAMILY_OPTS[dtype]
    armed = _copy(name, dtype, frozenset(opts))
    default = signature(_copy(name, dtype, frozenset()))
    singles = {o: signature(_copy(name, dtype, frozenset([o]))) for o in opts}
    units = _units(armed)
    rec = _record(armed, units, _input(res, batch))
    used = set()
    for names in units:
        x, want, want_paths = rec[tuple(names)]
        mine = frozenset(o for n in names for who in changed_by(default, singles, prefix=n).values() for o in who)
        used.add(mine)
        ref = _copy(name, dtype, mine)
        mods = [ref.get_submodule(n) for n in names]
        _reset_paths(*mods)
        with torch.inference_mode(), _pinned():
            y = x
            for m in mods:
                y = m(y)
        assert _unit_paths(mods) == want_paths, (names, sorted(mine), _unit_paths(mods), want_paths)
        assert y.dtype == want.dtype and y.shape == want.shape
        assert torch.equal(y, want), (names, sorted(mine), want_paths, float((y.float() - want.float()).abs().max()))
    assert len(used) >= 3 and frozenset(opts) not in used    # the references really are other copies


# ---- B: the class switches take the all-on copy back to the single-option copies

@pytest.mark.parametrize('name,res,batch', SETS)
def test_switch_lattice_f32(name, res, batch, hip_lib):
    armed = _copy(name, None, frozenset(F32_OPTS))
    x = _input(res, batch, seed=3)
    with _switched_off(F32_OPTS):
        got = _forward(armed, x)
    want = _forward(_copy(name, None, frozenset()), x)
    assert got[1] == want[1] and torch.equal(got[0], want[0])
    for o in F32_OPTS:
        with _switched_off([k for k in F32_OPTS if k != o]):
            got = _forward(armed, x)
        want = _forward(_copy(name, None, frozenset([o])), x)
        assert got[1] == want[1], (o, [(a, b) for a, b in zip(got[1], want[1]) if a != b])
        assert torch.equal(got[0], want[0]), (o, float((got[0] - want[0]).abs().max()))


def _block_paths_as_armed(armed, paths):
    """`paths` of a copy without fuse_blocks, as the all-on 16-bit copy reports them with K16h switched off: a FusedMBConv
    that holds a fused_pair says 'chain' for the two-kernel chain, where the same block without one says nothing (None).
    Every layer's own entry stays."""
    from metrabs_amd import backbones
    return ['chain' if isinstance(m, backbones.FusedMBConv) and m.fused_pair and p is None else p
            for m, p in zip(armed.modules(), paths)]


@pytest.mark.parametrize('dtype', [F16, BF16])
@pytest.mark.parametrize('name,res,batch', SETS)
def test_switch_lattice_16bit(name, res, batch, dtype, hip_lib):
    """deep_projects has no switch of its own: the base of the lattice is the deep_projects-only copy."""
    armed = _copy(name, dtype, frozenset(H16_OPTS))
    off = ('fuse_blocks', 'fuse_stem', 'block_depthwise')
    x = _input(res, batch, seed=3)
    with _switched_off(off):
        got = _forward(armed, x)
    want = _forward(_copy(name, dtype, frozenset(['deep_projects'])), x)
    assert torch.equal(got[0], want[0]) and got[1] == _block_paths_as_armed(armed, want[1])
    for o in off:
        with _switched_off([k for k in off if k != o]):
            got = _forward(armed, x)
        want = _forward(_copy(name, dtype, frozenset(['deep_projects', o])), x)
        assert torch.equal(got[0], want[0]), (o, float((got[0].float() - want[0].float()).abs().max()))
        want_paths = want[1] if o == 'fuse_blocks' else _block_paths_as_armed(armed, want[1])
        assert got[1] == want_paths, (o, [(a, b) for a, b in zip(got[1], want_paths) if a != b])


# ---- C: the accuracy of the all-on copies, by the criteria of the single options

@pytest.mark.parametrize('name', ['efficientnetv2-s', 'mobilenetv3'])
def test_all_on_f32_copy_accuracy_against_fp64(name, hip_lib):
    """128 px, B = 2, against an fp64 CPU forward of the same folded network: the all-on copy's relative RMS error is at
    most 2 x the default copy's (DESIGN.md section 22's margin for an option that differs by rounding; the criterion of
    the winograd3x3 and split_gemm copies alone).  Measured on an MI355X: DESIGN.md section 24."""
    plain = _copy(name, None, frozenset())
    nets = dict(plain=plain, winograd=_copy(name, None, frozenset(['winograd3x3'])),
                split=_copy(name, None, frozenset(['split_gemm'])), all=_copy(name, None, frozenset(F32_OPTS)))
    x = _input(128, 2, seed=4)
    ref = copy.deepcopy(plain).cpu().double()
    with torch.inference_mode():
        want = ref(x.cpu().double())
    err = {k: float((_forward(n, x)[0].double().cpu() - want).norm() / want.norm()) for k, n in nets.items()}
    paths = set(_all_paths(nets['all']))
    print(f'COMBO_NET {name} 128 px B = 2, relative RMS error against fp64: e_plain {err["plain"]:.4g} '
          f'e_winograd {err["winograd"]:.4g} e_split {err["split"]:.4g} e_all {err["all"]:.4g}')
    assert {'k17', 'k20', 'k20_gate'} <= paths and ('k19' in paths) == (name == 'efficientnetv2-s'), paths
    assert err['all'] <= 2 * err['plain'], err


@pytest.mark.parametrize('dtype', [F16, BF16])
@pytest.mark.parametrize('name', ['efficientnetv2-s', 'mobilenetv3'])
def test_all_on_16bit_copy_meets_the_default_copys_criteria(name, dtype, hip_lib):
    """256 px, B = 2: mean-abs and max-abs error against the f32 folded network, relative to the f32 copy under autocast
    of the same dtype (the criteria of tests/test_gpu_backbone16.py and test_gpu_backbone16_deep.py, factors unchanged)."""
    f32 = _copy(name, None, frozenset())
    armed = _copy(name, dtype, frozenset(H16_OPTS))
    x = _input(256, 2, seed=5)
    c, paths = _forward(armed, x)
    assert {'k17'} <= set(paths) and (name != 'efficientnetv2-s' or ('k16h' in paths and set(paths) & set(DEEP)))
    with torch.inference_mode(), _pinned():
        a = f32(x)
        with torch.autocast('cuda', dtype=dtype):
            b = f32(x)
    assert c.dtype == dtype and c.shape == a.shape and torch.isfinite(c).all()
    a = a.float()
    mean_c, mean_b = float((c.float() - a).abs().mean()), float((b.float() - a).abs().mean())
    amax = float(a.abs().max())
    max_c, max_b = float((c.float() - a).abs().max()), float((b.float() - a).abs().max())
    print(f'COMBO_NET16 {name} {dtype} 256 px B = 2: mean-abs {mean_c:.4g} (autocast {mean_b:.4g}), max-abs {max_c:.4g} '
          f'(autocast {max_b:.4g}), amax {amax:.4g}')
    assert mean_c <= 1.1 * mean_b + 1e-6 * amax, (mean_c, mean_b)
    if max_b <= 0.1 * amax:
        assert max_c <= 0.1 * amax, (max_c, max_b, amax)
    else:
        assert max_c <= 1.1 * max_b, (max_c, max_b, amax)


# ---- D: the loader and the API

def _api_inputs():
    images = torch.stack([cases.synth_images(1, 240, 320, 5 + i)[0] for i in range(2)]).cuda()
    boxes = [torch.tensor([[60.0, 20.0, 120.0, 200.0], [150.0, 30.0, 100.0, 180.0]]),
             torch.tensor([[40.0, 10.0, 140.0, 210.0]])]
    return images, boxes


def _poses(est, images, boxes, num_aug):
    with torch.inference_mode():
        return torch.cat(est.estimate_poses_batched(images, boxes, num_aug=num_aug)['poses3d']).clone()


def test_all_f32_options_through_the_loader_and_the_api(tmp_path, hip_lib):
    """Three crops through estimate_poses_batched: a graphed call returns the eager call's bits; MPJPE of the all-on model
    to the same folded network with its backbone evaluated in fp64 <= 2 x the default copy's."""
    from metrabs_amd import loading
    d = _model_dir(tmp_path)
    on = dict(fuse_stem=True, block_depthwise=True, winograd3x3=True, split_gemm=True)
    plain = loading.load_multiperson_model(d, fold_batchnorm=True, fused_epilogue=True)
    truth = loading.load_multiperson_model(d, fold_batchnorm=True, fused_epilogue=True)
    truth.crop_model.backbone = _Fp64Backbone(truth.crop_model.backbone)
    est = loading.load_multiperson_model(d, **on)
    eager = loading.load_multiperson_model(d, **on)
    for m in (plain, est, eager):
        m.crop_model.deterministic_backbone = True
    est.graph_batches, eager.graph_batches, truth.graph_batches = True, False, False
    images, boxes = _api_inputs()
    for _ in range(2):   # (the second call replays the graph)
        a, b = _poses(eager, images, boxes, 2), _poses(est, images, boxes, 2)
        assert torch.isfinite(a).all() and torch.equal(a, b), float((a - b).abs().max())
    st = est.graphs.stats
    assert st['captures'] >= 1 and st['replays'] >= 1, st
    for m in (est, eager):
        paths = set(_all_paths(m.crop_model.backbone))
        assert {'k17', 'k19', 'k20', 'k20_gate', 'k20_pre'} <= paths, paths
    p_true, p_plain, p_armed = (_poses(e, images, boxes, 1) for e in (truth, plain, eager))
    assert not {'k17', 'k18', 'k19', 'k20', 'k20_gate', 'k20_pre'} & set(_all_paths(plain.crop_model.backbone))
    mpjpe = lambda p, q: float((p - q).norm(dim=-1).mean())
    e_armed, e_plain = mpjpe(p_armed, p_true), mpjpe(p_plain, p_true)
    print(f'COMBO_NET MPJPE to the fp64-backbone poses: all-on copy {e_armed:.5g} mm, default copy {e_plain:.5g} mm; '
          f'all-on to default copy {mpjpe(p_armed, p_plain):.5g} mm')
    assert 0 < e_armed <= 2 * e_plain, (e_armed, e_plain)


def test_all_16bit_options_through_the_loader_and_the_api(tmp_path, hip_lib):
    """The f16 copy with all four options: graphed against eager, bit for bit, finite, on the armed paths (what
    test_deep_projects_through_the_loader_and_the_api asks of its copy)."""
    from metrabs_amd import backbones, loading
    d = _model_dir(tmp_path)
    ests = {}
    for key, graphed in [('graph', True), ('eager', False)]:
        est = loading.load_multiperson_model(d, dtype=F16, fuse_blocks=True, fuse_stem=True, block_depthwise=True,
                                             deep_projects=True)
        est.crop_model.deterministic_backbone = True
        est.graph_batches = graphed
        ests[key] = est
    images, boxes = _api_inputs()
    for _ in range(2):   # (the second call replays the graph)
        a, b = _poses(ests['eager'], images, boxes, 2), _poses(ests['graph'], images, boxes, 2)
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), float((a - b).abs().max())
    for key in ('graph', 'eager'):
        bb = ests[key].crop_model.backbone
        layers = [m for m in bb.modules() if isinstance(m, backbones.ConvBiasAct) and m.deep_projects]
        assert len(layers) == 15 and {m.last_path for m in layers} == {'k13h_deep_gate'}
        assert {'k16h', 'k17'} <= set(_all_paths(bb))
    st = ests['graph'].graphs.stats
    assert st['captures'] >= 1 and st['replays'] >= 1, st

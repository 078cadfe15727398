"""CPU: the shape fuzz of the backbone convolution kernels (tests/conv_fuzz.py) before it runs on a GPU.

  * every generated case is accepted: the C entry point, called with B = 0 on host buffers (the entries make all their
    argument checks before "B == 0: nothing to do"), returns 0, and the kernels.*_supported predicate answers True
    wherever it works on CPU tensors -- the generators construct their cases inside the domain, none is left out;
  * the draws reach the places the hand-picked shapes of the kernels' own modules do not: conditions on the INPUTS
    (tune the generator until they hold, never the test);
  * the checker can fail: each kernel's own bound accepts the fp64 reference rounded to the tensor's dtype and rejects
    four subtly wrong references wherever they differ from the right one by more than the bound.
"""
import math

import pytest
import torch

import conv_fuzz
from conv_fuzz import ACTS, KERNELS, MFMA, N_CASES


@pytest.fixture(scope='module')
def lib():
    from metrabs_amd import _lib
    return _lib.load()


def test_the_generators_are_deterministic_and_complete():
    assert list(KERNELS) == ['k13', 'k13h', 'k20', 'k14h', 'k19', 'k22', 'k16h', 'k17', 'k11', 'k15', 'k18', 'k10',
                             'se_gate']
    for name, k in KERNELS.items():
        assert len(k.cases()) == N_CASES
        assert type(k)().cases() == k.cases(), name   # a fixed seed of Python's generator
        assert len({conv_fuzz.case_id(c) for c in k.cases()}) == N_CASES, name


@pytest.mark.parametrize('name', list(KERNELS))
def test_every_generated_case_is_accepted(name, lib):
    k = KERNELS[name]
    with_predicate = 0
    for i, c in enumerate(k.cases()):
        codes = k.accept(lib, c)
        assert codes and all(rc == 0 for rc in codes), (name, i, c, codes)
        ok = k.supported(c)
        assert ok is None or ok is True, (name, i, c)
        with_predicate += ok is not None
    assert with_predicate in (0, N_CASES)   # the share of cases left out is zero


def test_the_cases_outside_the_domains_break_one_rule_of_an_accepted_case(lib):
    """tests/test_gpu_conv_fuzz.py breaks one rule at a time of these smallest cases: as they stand they are accepted."""
    assert sorted(conv_fuzz.OUTSIDE) == sorted(KERNELS)
    for name, (base, broken) in conv_fuzz.OUTSIDE.items():
        k = KERNELS[name]
        assert all(rc == 0 for rc in k.accept(lib, base)), name
        assert k.supported(base) in (None, True), name
        assert len(broken) >= 2 and all(code in (-2, -4, -6) for *_, code in broken), name
        for what, changed, shift_x, shift_y, _ in broken:
            assert (len(changed) >= 1) != bool(shift_x or shift_y), (name, what)   # one thing at a time


# ---- the draws

def _options_both_ways(name, cases, keys):
    for key in keys:
        values = {bool(c[key]) for c in cases}
        assert values == {False, True}, (name, key, values)


@pytest.mark.parametrize('name', MFMA)
def test_the_mfma_draws_reach_partial_channel_tiles_and_odd_maps(name):
    from metrabs_amd import kernels
    k, cases = KERNELS[name], KERNELS[name].cases()
    couts = [c['M'] for c in cases]
    assert sum(m % 8 != 0 for m in couts) >= 8, couts           # a partial last fragment of 16 or 32 rows
    assert sum(m < 8 for m in couts) >= 3 and 1 in couts, couts
    tiles = [k.tiles(kernels, c) for c in cases]
    # K16h holds all of Cout (<= 128) in one workgroup: what it walks in tiles is Cmid
    chans = [c['Cmid'] if name == 'k16h' else c['M'] for c in cases]
    assert sum(ch > bm and ch % bm != 0 for ch, (bm, _) in zip(chans, tiles)) >= 3, list(zip(chans, tiles))
    assert sum(c['H'] != c['W'] for c in cases) >= 8
    unit = 4 if name == 'k19' else 1   # K19's columns are Winograd tiles of 2 x 2 outputs
    below = spans = partial = 0
    for c, (_, bn) in zip(cases, tiles):
        per_image = math.prod(k.out_shape(c)[2:]) // unit
        if k.joint_columns:
            below += c['B'] * per_image < bn // unit
            spans += conv_fuzz.tile_spans_two_images(c['B'], per_image, bn // unit)
        else:   # the grid has the image as a dimension of its own: a tile never spans two
            below += per_image < bn
            partial += c['B'] >= 2 and per_image % bn != 0
    assert below >= 3, below
    assert (spans if k.joint_columns else partial) >= 3, (spans, partial)
    assert {c['act'] for c in cases} == set(ACTS)
    _options_both_ways(name, cases, [key for key in ('gate', 'residual', 'in_bias') if key in cases[0]])
    if 'in_bias' in cases[0]:
        assert {c['in_act'] for c in cases if c['in_bias']} == set(ACTS)
        assert all(c['in_act'] is None for c in cases if not c['in_bias'])
    assert {c['dtype'] for c in cases} == set(getattr(k, 'dtypes', None) or {c['dtype'] for c in cases})
    if name in ('k14h', 'k16h'):
        assert {c['stride'] for c in cases} == {1, 2} and {c['dtype'] for c in cases} == {torch.float16, torch.bfloat16}
    if name == 'k16h':
        assert {c['residual'] for c in cases} == {None, 'x', 'other'}
        assert any(c['chain'] for c in cases) and any(not c['chain'] for c in cases)
    if name in ('k13', 'k13h'):   # K of 400 and more: the deep-K rings of three stages wrap
        assert sum(c['K'] >= 400 for c in cases) >= 3
        named = {cfg for c in cases for cfg in k.configs(kernels, c)}
        assert named == {'auto'} | set(k.CONFIGS), named


@pytest.mark.parametrize('name', ['k11', 'k15', 'k18', 'k10'])
def test_the_depthwise_and_k10_draws(name):
    cases = KERNELS[name].cases()
    chans = [c['C'] for c in cases]
    assert 1 in chans and sum(ch % 2 == 1 for ch in chans) >= 8, chans
    assert {c['act'] for c in cases} == set(ACTS)
    assert {c['dtype'] for c in cases} == {torch.float32, torch.float16, torch.bfloat16}
    _options_both_ways(name, cases, ['want_mean'] + (['residual'] if name == 'k10' else []))
    if name in ('k11', 'k15'):   # the two entries that allow it: K18 asks for W % 4 == 0, K10 for whole 16-byte vectors
        assert sum(c['H'] * c['W'] % 4 != 0 for c in cases) >= 3
        assert {c['stride'] for c in cases} == {1, 2}
        assert {(c['stride'], c['pad']) for c in cases} == set(KERNELS[name].VARIANTS)
    if name == 'k11':
        from metrabs_amd import kernels
        assert sum(c['stride'] == 1 and c['pad'] == (1, 1, 1, 1) and kernels.k11_takes_block_kernel(c['H'], c['W'])
                   for c in cases) >= 2
    if name == 'k18':
        assert {c['block_cols'] for c in cases} == {None, 4, 8}


def test_the_stem_and_gate_draws():
    stem = KERNELS['k17'].cases()
    assert {(c['xdtype'], c['dtype']) for c in stem} == set(KERNELS['k17'].PAIRS)
    assert {c['act'] for c in stem} == set(ACTS) and sum(c['H'] != c['W'] for c in stem) >= 8
    _options_both_ways('k17', stem, ['preproc', 'interleaved'])
    gate = KERNELS['se_gate'].cases()
    assert {(c['act'], c['gate_fn']) for c in gate} == set(KERNELS['se_gate'].PAIRS)
    assert {c['config'] for c in gate} == {-1, 0, 1, 2, 3} and 1 in [c['S'] for c in gate]
    _options_both_ways('se_gate', gate, ['w2t'])


# ---- the checker

def _rejects(k, c, inp, got):
    try:
        k.check(c, inp, got)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize('name', list(KERNELS))
def test_the_checker_accepts_the_reference_and_rejects_wrong_ones(name, capsys):
    """`got` = the fp64 reference rounded to the tensor's dtype passes the kernel's own check.  A wrong reference,
    rounded the same way, MUST be rejected where it lies further from the right one than the bound plus its own
    rounding somewhere (then |got - ref| > bound there, whatever the rounding did); counted per kind of mistake.  A
    left-out channel and a swapped pair of taps move every output by orders of magnitude more than a bound of a few
    units in the last place, so each must be rejected on every case it applies to."""
    k = KERNELS[name]
    applicable, rejected = {}, {}
    for i, c in enumerate(k.cases()):
        inp = k.inputs(c, 'cpu', seed=i)
        ref, bound = k.reference(c, inp)
        out_dtype = c['dtype']
        assert tuple(ref.shape) == tuple(k.out_shape(c)), (name, i)
        assert not _rejects(k, c, inp, ref.to(out_dtype).contiguous()), (name, i, c)
        for kind, wrong in k.wrong(c, inp).items():
            got = wrong.to(out_dtype).contiguous()
            must = bool(((wrong - ref).abs() > bound + (got.double() - wrong).abs()).any())
            applicable[kind] = applicable.get(kind, 0) + 1
            if must:
                assert _rejects(k, c, inp, got), (name, i, kind, c)
                rejected[kind] = rejected.get(kind, 0) + 1
    with capsys.disabled():
        print(f'\nCHECKER_SELF_TEST {name}: rejected / applicable {[(kind, rejected.get(kind, 0), n) for kind, n in applicable.items()]}')
    for kind in ('last_channel', 'taps_swapped'):
        if kind in applicable:
            assert rejected.get(kind, 0) == applicable[kind], (name, kind, rejected.get(kind, 0), applicable[kind])
    # (a relu hides a shifted bias where the last channel is negative at every position of a tiny map, two neighbouring
    # biases may lie within a bf16 bound of each other, and a skip in front of a relu changes nothing where the sums are
    # positive: wherever they differ by more than the bound, which is most cases and not every one)
    for kind in ('bias_shift', 'residual_first'):
        if kind in applicable:
            assert 2 * rejected.get(kind, 0) >= applicable[kind], (name, rejected, applicable)
    assert set(applicable) == set(WRONG_KINDS[name]), (name, applicable)


_GEMM, _DENSE = ['last_channel', 'bias_shift', 'residual_first'], ['last_channel', 'taps_swapped', 'bias_shift']
# which mistakes a kernel's operation can hold: no taps in a 1x1 convolution, no input-channel sum in a depthwise one,
# no activation behind K16h's project, no skip in K17, K11, K15, K18 and the gate
WRONG_KINDS = {'k13': _GEMM, 'k13h': _GEMM, 'k20': _GEMM, 'k14h': _DENSE + ['residual_first'],
               'k19': _DENSE + ['residual_first'], 'k22': _DENSE + ['residual_first'], 'k16h': _DENSE, 'k17': _DENSE,
               'k11': ['taps_swapped', 'bias_shift'], 'k15': ['taps_swapped', 'bias_shift'],
               'k18': ['taps_swapped', 'bias_shift'], 'k10': ['bias_shift', 'residual_first'],
               'se_gate': ['last_channel', 'bias_shift']}

"""CPU: the generator, the yardstick and the checker of tests/filter_fuzz.py (K8, the plausibility filter + pose NMS,
24 seeded calls whose decisions are PLACED a small, known distance from their thresholds).  Nothing here launches a
kernel:

  * the generator is deterministic; every balanced value, every class and both sides of every class occur; the pose
    counts 0 .. 5 and 12, an empty image first, in the middle and last, invalid poses between valid ones;
  * at the default parameters the yardstick's masks and kept lists equal cpu_ref.filter_poses on float64 copies of the
    inputs, for both orders; cpu_ref.filter_poses on the float32 inputs decides the same in every such case; the
    float32 oracle's similarity lies inside the similarity bound (with the counts of an f32 evaluation);
  * margin(case) >= 8 for every case (printed), and DELTA_PAIR is the smallest power of two that gets the pairs there;
  * every kind of filter_fuzz.WRONG changes a decision or breaks a bound in at least one case; the yardstick passes;
  * the entry's rules without a launch (n_images = 0): the dynamic LDS limit from both sides, A = 0, J_model."""
import ctypes

import numpy as np
import pytest
import torch

import filter_fuzz as ff
from oracle import cpu_ref

MTR_OK, MTR_E_SHAPE, MTR_E_PARAM = 0, -2, -4


@pytest.fixture(scope='module')
def refs():
    return [ff.yardstick(c) for c in ff.cases()]


def test_generator_is_deterministic_and_reaches_everything():
    cs = ff.cases()
    again = ff.build_case(5)
    for k in ('poses3d', 'poses2d', 'boxes', 'mean_bones'):
        assert again[k].tobytes() == cs[5][k].tobytes()
    assert again['classes'] == cs[5]['classes'] and len(cs) == ff.N_CASES == 24
    assert {c['J'] for c in cs} == set(ff.J_VALUES) and {c['A'] for c in cs} == set(ff.A_VALUES)
    assert {c['skeleton'] for c in cs} == set(ff.SKELETONS)
    assert {(c['order_by_score'], c['var_correction'], c['alt']) for c in cs} == {(o, v, a) for o in (0, 1) for v in (0, 1)
                                                                                  for a in (0, 1)}
    assert any(len(c['edges']) > 64 and c['J'] < 64 for c in cs) and any(len(c['edges']) > 64 and c['J'] >= 122 for c in cs)
    assert {(c['A'], c['var_correction']) for c in cs} >= {(1, 0), (1, 1)}
    for c in cs:
        assert 1 <= len(c['counts']) <= 5 and c['poses3d'].shape == (sum(c['counts']), c['A'], c['J'], 3)
        assert c['poses3d'].dtype == c['poses2d'].dtype == c['boxes'].dtype == np.float32
        if c['A'] == 65 or c['J'] >= 122:
            assert sum(c['counts']) <= 6
        inside = [a < c['J_model'] and b < c['J_model'] for a, b in c['edges']]
        assert all(inside) or c['skeleton'] == 'chain_past'
        if c['J_model'] < c['J']:
            assert float(np.abs(c['poses3d'][:, :, c['J_model']:]).min()) >= 9e4
        assert float(np.abs(c['poses2d'] * 64 - np.round(c['poses2d'] * 64)).max()) == 0 and float(c['poses2d'].max()) < 2048
    counts = [n for c in cs for n in c['counts']]
    assert set(counts) >= {0, 1, 2, 3, 4, 5, 12}
    assert any(c['counts'][0] == 0 for c in cs) and any(c['counts'][-1] == 0 for c in cs)
    assert any(0 in c['counts'][1:-1] for c in cs)
    classes = {cl[:3] if cl[0] == 'box' else cl[:2] for c in cs for cl in c['classes']}
    want = {('bone%d' % b, s) for b in (1, 2, 3, 4) for s in (1, -1)} | {('stdev', 1), ('stdev', -1)} | \
        {('box', ax, s) for ax in (0, 1) for s in (1, -1)} | {('pair%d' % p, s) for p in (1, 2, 3) for s in (1, -1)} | \
        {('chain', o) for o in (0, 1, 2)} | {('box_eq',), ('plain',)}
    assert classes == want, classes ^ want


def test_classes_decide_as_placed(refs):
    """Each placed pose gets the decision its side says, and the chains keep what their score order says."""
    interleaved = False
    for c, y in zip(ff.cases(), refs):
        nan_case = c['A'] == 1 and c['var_correction'] == 1
        for q, cl in enumerate(c['classes']):
            if nan_case:
                assert not y['valid'][q] and np.isnan(y['sd'][q]).all()
                continue
            if cl[0].startswith('bone'):
                bad_side = -1 if cl[0] == 'bone3' else 1       # bone3: BELOW rel_small is out of range
                assert y['plausible'][q] == (cl[1] != bad_side) and y['consistent'][q] and y['in_box'][q], (c['index'], q, cl)
            elif cl[0] == 'stdev':
                assert y['consistent'][q] == (cl[1] == -1) and y['n_stable'][q] == c['J'] // 4 + (cl[1] == -1)
            elif cl[0] == 'box':
                assert y['in_box'][q] == (cl[2] == 1) and y['plausible'][q] and y['consistent'][q]
            elif cl[0] == 'box_eq':
                assert not y['in_box'][q] and y['box']['area'][q] == y['box_thr'][q] > 0
            else:
                assert y['valid'][q], (c['index'], q, cl)
        for i, (lo, hi) in enumerate(zip(c['row_start'][:-1], c['row_start'][1:])):
            idx = y['valid_lists'][i]
            interleaved |= bool(idx) and idx != list(range(lo, lo + len(idx))) and max(idx) - min(idx) + 1 > len(idx)
            where = {c['classes'][q][1:]: q for q in range(lo, hi) if c['classes'][q][0] == 'chain'}
            for o in (0, 1, 2):
                if (o, 'A') in where and not nan_case:
                    a, b, cc = (where[(o, n)] for n in 'ABC')
                    kept = [q for q in y['kept'][1][i] if q in (a, b, cc)]
                    if len(y['kept'][1][i]) < y['params']['max_output']:
                        assert kept == {0: [a, cc], 1: [b], 2: [cc, a]}[o], (c['index'], o, kept)
            for q in range(lo, hi):
                cl = c['classes'][q]
                if cl[0].startswith('pair') and cl[2] == 'u' and not nan_case:
                    v = next(r for r in range(lo, hi) if c['classes'][r] == (cl[0], cl[1], 'v') and r != q)
                    s = y['sim'][i][idx.index(q), idx.index(v)]
                    thr = y['params']['sim_threshold']
                    assert abs(s / thr - 1 - cl[1] * ff.DELTA_PAIR) < 2.0 ** -15, (c['index'], cl, s)
    assert interleaved


def test_yardstick_agrees_with_the_oracle_at_the_default_parameters(refs):
    n = 0
    for c, y in zip(ff.cases(), refs):
        if c['alt']:
            continue
        n += 1
        k = c['J'] // 4
        for dtype in (torch.float64, torch.float32):
            boxes, p3, p2, edges, mb = ff.torch_inputs(c, dtype)
            for order in (0, 1):
                keep, masks = cpu_ref.filter_poses(boxes, p3, p2, edges, mb, n_joints=c['J_model'],
                                                   unbiased=bool(c['var_correction']), order='score' if order else 'index')
                for i, lo in enumerate(c['row_start'][:-1]):
                    hi = c['row_start'][i + 1]
                    assert masks[i].tolist() == y['valid'][lo:hi].tolist(), (c['index'], dtype, i)
                    assert [lo + int(q) for q in keep[i]] == y['kept'][order][i], (c['index'], dtype, order, i)
        for i, idx in enumerate(y['valid_lists']):          # the f32 oracle's similarity, from the same f32 mean poses
            if len(idx) and k:
                got = cpu_ref.compute_pose_similarity(torch.from_numpy(y['mean32'][idx])).double().numpy()
                bound = ff.sim_bound(y['l1'][i], y['params']['sim_scale_mm'], scale_u=ff.scale_u_f32(c['J']), mean_u=k)
                assert np.all(np.abs(got - y['sim'][i]) <= bound), (c['index'], i)
    assert n == 13


def test_every_margin_is_at_least_8(refs):
    margins = [ff.margin(c, y) for c, y in zip(ff.cases(), refs)]
    print('FILTER_FUZZ margins', ' '.join('%.1f' % m for m in margins), 'smallest %.2f' % min(margins))
    assert min(margins) >= 8
    # the pair classes at 2^-12 would not get there: DELTA_PAIR is the smallest power of two that does
    assert ff.DELTA_PAIR == 2 * ff.DELTA
    worst = min(abs(y['sim'][i][a, b] - y['params']['sim_threshold']) / ff.sim_bound(y['l1'][i], y['params']['sim_scale_mm'])[a, b]
                for c, y in zip(ff.cases(), refs) for i in range(len(y['sim'])) for a in range(len(y['sim'][i]))
                for b in range(a) if not np.isnan(y['sim'][i][a, b]))
    assert 8 <= worst < 16, worst


def test_the_checker_passes_the_yardstick_and_catches_every_wrong_kind(refs):
    for c, y in zip(ff.cases(), refs):
        fails, shares = ff.check(c, y, ff.answer(c, y))
        assert not fails and shares['sim'] < 0.1      # (answer() rounds the similarity to f32)
    for kind in ff.WRONG:
        caught = [c['index'] for c, y in zip(ff.cases(), refs) if ff.check(c, y, ff.wrong(kind, c))[0]]
        print('FILTER_FUZZ wrong', kind, 'caught in cases', caught)
        assert caught, kind


def test_entry_rules_without_a_launch(hip_lib):
    """n_images = 0: the entry checks its shape and parameter rules and launches nothing.  The dynamic LDS request is
    16 * (J rounded up to even) + 32 * A bytes (4 waves of J float distances and of A double factors); 48 KiB is the
    limit: with A = 1, J = 3070 asks for 49 152 bytes and J = 3071 for 49 184."""
    from metrabs_amd import _lib
    fp = _lib.FilterParams(0.1, 3.0, 300.0, 200.0, 0.5, 300.0, 0.4, 150, 0, 1)

    def call(A, J, J_model=None, max_per_image=1):
        return hip_lib.mtr_filter_poses(None, None, None, None, None, 0, 0, A, J, None, None, 0, J if J_model is None else J_model,
                                        ctypes.byref(fp), None, 0, max_per_image, None, None, None, None)

    lds = lambda A, J: 16 * ((J + 1) & ~1) + 32 * A
    assert lds(1, 3070) == 48 * 1024 and lds(1, 3071) > 48 * 1024
    assert call(1, 3070) == MTR_OK and call(1, 3071) == MTR_E_SHAPE
    assert call(2, 3068) == MTR_OK and call(2, 3069) == MTR_E_SHAPE and call(3, 3068) == MTR_E_SHAPE
    assert call(65, 129) == MTR_OK
    assert call(0, 17) == MTR_E_SHAPE and call(1, 0) == MTR_E_SHAPE
    assert call(1, 17, J_model=0) == MTR_E_PARAM and call(1, 17, J_model=18) == MTR_E_PARAM
    assert call(1, 17, J_model=1) == MTR_OK and call(1, 17, J_model=17) == MTR_OK
    assert call(1, 17, max_per_image=1025) == MTR_E_SHAPE and call(1, 17, max_per_image=1024) == MTR_OK

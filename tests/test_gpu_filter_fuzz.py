"""GPU: K8 (mtr_filter_poses) on the 24 seeded calls of tests/filter_fuzz.py, whose decisions are PLACED a small, known
distance from their thresholds (tests/test_filter_fuzz_host.py holds the generator to its classes, the yardstick to
the oracle, every margin to >= 8 bounds and the checker to rejecting fifteen subtly wrong kernels).  Per case, through
the C-ABI with the caller's own NaN-filled workspace read back:

  * the mean poses: the bits of the in-order float32 loop, and inside the fp64 bound;
  * every similarity block: inside the derived bound, symmetric bit for bit, compact nv x nv; the workspace floats
    past an image's nv^2 still hold the prefill;
  * valid, keep_idx, keep_count equal to the fp64 yardstick exactly; -1 behind each image's kept rows; guard bands intact;
  * image i of the call carries the bits of a call on that image alone; three calls give equal bits.

One FILTER_FUZZ line per case: the shape, the largest share of each bound used, the margin.  Then three default-
parameter cases through the Python wrapper, and one launch at the largest dynamic LDS request the entry accepts."""
import numpy as np
import pytest
import torch

import filter_fuzz as ff

pytestmark = pytest.mark.gpu


def _same(a, b):
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize('i', range(ff.N_CASES))
def test_filter_fuzz_case(i, hip_lib):
    c = ff.case(i)
    y = ff.yardstick(c)
    got = ff.run(hip_lib, c)
    assert got['code'] == 0
    fails, shares = ff.check(c, y, got)
    print('FILTER_FUZZ case %d J=%d A=%d J_model=%d %s bones=%d images=%s order=%d var_correction=%d alt=%d valid=%d/%d '
          'mean_share=%.3f sim_share=%.3f margin=%.1f' % (i, c['J'], c['A'], c['J_model'], c['skeleton'], len(c['edges']),
                                                          c['counts'], c['order_by_score'], c['var_correction'], c['alt'],
                                                          int(y['valid'].sum()), len(y['valid']), shares['mean'],
                                                          shares['sim'], ff.margin(c, y)))
    assert not fails, fails
    for _ in range(2):                                              # three calls, equal bits
        again = ff.run(hip_lib, c)
        assert again['code'] == 0 and again['bands']
        assert all(_same(again[k], got[k]) for k in ('valid', 'keep_idx', 'keep_count', 'mean'))
        assert all(_same(a, b) for a, b in zip(again['sim'], got['sim']))
    for im, (lo, hi) in enumerate(zip(c['row_start'][:-1], c['row_start'][1:])):     # each image alone
        if hi == lo or len(c['counts']) == 1:
            continue
        alone = ff.run(hip_lib, ff.sub_case(c, im))
        assert alone['code'] == 0 and alone['bands']
        assert _same(alone['valid'], got['valid'][lo:hi]) and _same(alone['mean'], got['mean'][lo:hi])
        assert _same(alone['sim'][0], got['sim'][im]) and alone['keep_count'][0] == got['keep_count'][im]
        assert np.where(alone['keep_idx'] >= 0, alone['keep_idx'] + lo, -1).tolist() == got['keep_idx'][lo:hi].tolist()


@pytest.mark.parametrize('i', [0, 3, 17])
def test_the_python_wrapper_decides_the_same(i, hip_lib):
    """metrabs_amd.kernels.filter_poses (default parameters; its own workspace and outputs)."""
    from metrabs_amd import kernels
    c = ff.case(i)
    assert not c['alt']
    want = ff.answer(c, ff.yardstick(c))
    keep_idx, keep_count, valid = kernels.filter_poses(
        torch.from_numpy(c['poses3d']).cuda(), torch.from_numpy(c['poses2d']).cuda(), torch.from_numpy(c['boxes']).cuda(),
        c['counts'], c['edges'] or None, torch.from_numpy(c['mean_bones']) if c['edges'] else None, n_joints=c['J_model'],
        unbiased=bool(c['var_correction']), order='score' if c['order_by_score'] else 'index')
    assert valid.cpu().tolist() == want['valid'].astype(bool).tolist()
    assert keep_count.cpu().tolist() == want['keep_count'].tolist() and keep_idx.cpu().tolist() == want['keep_idx'].tolist()


def test_the_largest_dynamic_lds_request_the_entry_accepts(hip_lib):
    """J = 3070, A = 1: 16 * 3070 + 32 = 49 152 bytes of dynamic LDS, the entry's limit, on top of the kernel's static
    tables (five of 1024 words: 20 KiB) -- about 68 KiB of the 160 KiB of a CU.  Two poses, an exact-duplicate pair: both
    valid, similarity exactly 1, the lower score goes."""
    rng = np.random.default_rng(3070)
    J = 3070
    one = (rng.standard_normal((1, 1, J, 3)) * 300 + np.array([100.0, -200.0, 2500.0])).astype(np.float32)
    p2 = (np.round((rng.random((1, 1, J, 2)) * np.array([300.0, 500.0]) + 400.0) * 64) / 64).astype(np.float32)
    lo, hi = p2[0, 0].min(axis=0), p2[0, 0].max(axis=0)
    box = [lo[0] - 8, lo[1] - 8, hi[0] - lo[0] + 16, hi[1] - lo[1] + 16]
    c = dict(index=-1, J=J, A=1, J_model=J, skeleton='none', order_by_score=1, var_correction=0, alt=0,
             params=dict(ff.DEFAULTS), edges=[], mean_bones=np.zeros(0, np.float32), counts=[2], row_start=[0, 2],
             classes=[('plain',), ('plain',)], poses3d=np.repeat(one, 2, axis=0), poses2d=np.repeat(p2, 2, axis=0),
             boxes=np.array([box + [0.4], box + [0.7]], np.float32))
    y = ff.yardstick(c)
    assert y['valid'].tolist() == [True, True] and y['kept'][1] == [[1]] and float(y['sim'][0][0, 1]) == 1.0
    got = ff.run(hip_lib, c)
    assert got['code'] == 0, 'the entry accepted a launch the runtime refuses: code %d' % got['code']
    fails, shares = ff.check(c, y, got)
    assert not fails, fails
    assert got['sim'][0].tolist() == [1.0] * 4 and got['keep_idx'].tolist() == [1, -1] and got['keep_count'].tolist() == [1]

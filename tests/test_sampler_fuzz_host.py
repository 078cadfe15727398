"""CPU: the fuzz of the crop sampler (tests/sampler_fuzz.py) before it runs on a GPU.

  * the generators are deterministic and complete: every frame class and every row class of the issue is populated;
  * the fp64 yardstick (the row's formula with direct pixel coordinates) equals the oracle evaluated in float64 to 1e-12
    wherever every side of the level is at least 2 -- where a side is 1 the oracle returns NaN and the direct formula is
    the specification;
  * the checker can pass and can fail: it accepts the oracle's own f32 evaluation and a second, independent one (the
    direct formula in float32: the 4x margin is feasible for an honest f32 sampler), and rejects every wrong variant on
    at least one row of every frame set where the variant applies (tune the generator until it does, never the checker);
  * the geometry cases cover every box, camera and up-vector class, the oracle's fp64 look-at takes the fallback branch on
    the cases made for it, and the hand-made scales land on both sides of the level thresholds.
"""
import numpy as np
import pytest
import torch

import sampler_fuzz as sf
from oracle import cpu_ref

SETS = sf.frame_sets()
IDS = [fs['name'] for fs in SETS]
_CACHE = {}


def evaluated(fs):
    """(levels, truth64, ref32) of a frame set, computed once and left unchanged."""
    if fs['name'] not in _CACHE:
        lin = (sf.frames_of(fs).float() / 255) ** 2.2
        levels = sf.cpu_pyramid(lin)
        with torch.inference_mode():
            truth = [sf.yardstick(levels, r) for r in fs['rows']]
            ref = [sf.reference32(levels, r) for r in fs['rows']]
        _CACHE[fs['name']] = (levels, truth, ref)
    return _CACHE[fs['name']]


def test_the_generators_are_deterministic_and_complete():
    again = [sf._build_set(i, *shape) for i, shape in enumerate(sf.FRAME_SETS)]
    for a, b in zip(SETS, again):
        assert all(np.array_equal(x['wp'], y['wp']) and x['cls'] == y['cls'] for x, y in zip(a['rows'], b['rows']))
    assert 11 <= len(SETS) <= 14 and len(set(IDS)) == len(SETS)
    shapes = [(fs['n'], fs['h'], fs['w']) for fs in SETS]
    assert all(1 <= n <= 3 and max(h, w) <= 200 for n, h, w in shapes) and {n for n, _, _ in shapes} == {1, 2, 3}
    for cls4 in range(4):   # each class of W % 4 at least twice, also among the frames the row-walking kernel takes
        assert sum(w % 4 == cls4 for _, _, w in shapes) >= 2
        assert sum(w % 4 == cls4 and sf.uses_rows_kernel(h, w, 1) for _, h, w in shapes) >= 2
    assert sum(h % 8 == 0 and w % 8 == 0 for _, h, w in shapes) >= 2      # the wide pyramid kernel
    assert sum(h % 8 != 0 or w % 8 != 0 for _, h, w in shapes) >= 2
    assert sum(h % 2 == 1 for _, h, _ in shapes) >= 3
    two = [s for s in shapes if 8 <= min(s[1:]) <= 11]
    assert any(h < w for _, h, w in two) and any(w < h for _, h, w in two)   # two rows / two columns on level 2
    assert all(min(sf.level_dims(h, w)[2]) == 2 and sf.uses_rows_kernel(h, w, 1) for _, h, w in two)
    one = [s for s in shapes if 4 <= min(s[1:]) <= 7]
    assert len(one) >= 2 and all(min(sf.level_dims(h, w)[2]) == 1 and not sf.uses_rows_kernel(h, w, 1) for _, h, w in one)
    tiny = [s for s in shapes if 2 <= min(s[1:]) <= 3]
    assert len(tiny) >= 2 and all(min(sf.level_dims(h, w)[1]) == 1 and min(sf.level_dims(h, w)[2]) == 0 for _, h, w in tiny)


@pytest.mark.parametrize('fs', SETS, ids=IDS)
def test_every_row_class_is_populated(fs):
    rows = fs['rows']
    assert 16 <= len(rows) <= 24 and len(rows) % 8 != 0
    for g in range(3):
        idx, wp, res, aa = sf.group_rows(fs, g)
        assert len(idx) % 8 != 0 and wp.shape == (len(idx), 36) and res in sf.RES and aa in sf.AAS
    assert max(len(sf.group_rows(fs, g)[0]) for g in range(3)) > 8   # a launch with a second block of eight crops
    classes = [r['cls'] for r in rows]
    for cls in sf.CLASSES:
        assert classes.count(cls) >= 1, cls
    assert sum(r['rot'] for r in rows) >= 1 and sum(r['flip'] for r in rows) >= 1 and sum(r['persp'] for r in rows) >= 1
    last = [r for r in rows if r['cls'] == 'last_br']
    assert all(r['img'] == fs['n'] - 1 for r in last)
    live = [l for l in range(3) if min(fs['dims'][l]) >= 1]
    assert {r['level'] for r in rows} == set(live)
    assert all(r['img'] < fs['n'] and min(fs['dims'][r['level']]) >= 1 for r in rows)
    assert {r['dist'] for r in rows} == {'none', 'd5', 'd12'}
    ones = sum(r['gexp'] == 1.0 for r in rows)
    assert abs(2 * ones - len(rows)) <= 1 and all(0.25 < r['gexp'] < 0.42 for r in rows if r['gexp'] != 1.0)
    for i, r in enumerate(rows):   # signs drawn, magnitudes at most the fixtures'
        limit = np.abs(np.array({'none': [0] * 12, 'd5': list(sf.cases.DISTORTION_5) + [0] * 7,
                                 'd12': sf.cases.DISTORTION_12}[r['dist']], dtype=np.float32))
        assert (np.abs(r['wp'][18:30]) <= limit).all() and r['wp'][30] == float(r['dist'] != 'none')
        sf._assert_domain_and_class(r, fs['dims'], fs['n'])
    if sf.uses_rows_kernel(fs['h'], fs['w'], 1):
        assert {r['kernel'] for r in rows} == {'rows', 'taps'}
    else:
        assert {r['kernel'] for r in rows} == {'taps'}


def test_the_launches_cover_every_resolution_and_antialias_factor_on_both_kernels():
    seen = {(fs['groups'][g][0], fs['groups'][g][1], sf.kernel_pool(fs['h'], fs['w'], fs['groups'][g][1]))
            for fs in SETS for g in range(3)}
    assert {r for r, _, _ in seen} == set(sf.RES) and {a for _, a, _ in seen} == set(sf.AAS)
    for kernel in ('rows', 'taps'):
        assert {r % 4 for r, _, k in seen if k == kernel} == {0, 1, 2, 3}, kernel   # 7, 18 / 30, 33 and the multiples of 4
    assert any(k == 'taps' and a == 1 for _, a, k in seen) and any(k == 'taps' and a == 4 for _, a, k in seen)
    # u8 windows: level-0 rows on frames of every W % 4, through the row-walking kernel
    for cls4 in range(4):
        assert any(r['level'] == 0 and r['kernel'] == 'rows' for fs in SETS if fs['w'] % 4 == cls4 for r in fs['rows'])


@pytest.mark.parametrize('fs', SETS, ids=IDS)
def test_the_yardstick_is_the_oracle_in_float64(fs):
    levels, truth, _ = evaluated(fs)
    compared = 0
    for r, t in zip(fs['rows'], truth):
        with torch.inference_mode():
            o64 = sf.oracle(levels, r, eval_dtype=torch.float64)
        if sf.has_degenerate_side(levels, r):
            assert not bool(torch.isfinite(o64).all())   # the oracle divides by size - 1 = 0: no answer there
            assert bool(torch.isfinite(t).all())
            continue
        compared += 1
        assert float((o64 - t).abs().max()) <= 1e-12, r['cls']
    assert compared >= len(fs['rows']) // 2
    assert all(bool((t == 0).all()) for r, t in zip(fs['rows'], truth) if r['cls'] == 'outside')


@pytest.mark.parametrize('fs', SETS, ids=IDS)
def test_the_checker_accepts_two_honest_f32_evaluations(fs):
    levels, truth, ref = evaluated(fs)
    rep = sf.check(fs['name'], fs['rows'], ref, truth, ref)
    assert rep.ok, rep.failures
    with torch.inference_mode():
        direct = [sf.direct32(levels, r) for r in fs['rows']]
    rep = sf.check(fs['name'], fs['rows'], direct, truth, ref)
    print('\n'.join(rep.lines))
    assert rep.ok and not rep.bad_rows, rep.failures


@pytest.mark.parametrize('variant', sf.WRONG)
def test_the_checker_rejects_every_wrong_variant_on_every_frame_set(variant):
    for fs in SETS:
        levels, truth, ref = evaluated(fs)
        rows = [i for i in range(len(fs['rows'])) if sf.wrong_applies(variant, fs, i)]
        assert rows or variant == 'next_image' and fs['n'] == 1, (variant, fs['name'])
        if not rows:
            continue
        ours = [t.clone() for t in ref]
        with torch.inference_mode():
            for i in rows:
                ours[i] = sf.wrong(variant, fs, levels, i)
        rep = sf.check(fs['name'], fs['rows'], ours, truth, ref)
        assert not rep.ok and set(rep.bad_rows) & set(rows), (variant, fs['name'])
        assert set(rep.bad_rows) <= set(rows), (variant, fs['name'])   # and only rows that are wrong


def test_the_checker_wants_exact_zeros_outside_the_frame():
    fs = SETS[0]
    _, truth, ref = evaluated(fs)
    i = [r['cls'] for r in fs['rows']].index('outside')
    ours = [t.clone() for t in ref]
    ours[i][0, 0, 0] = 1e-30
    rep = sf.check(fs['name'], fs['rows'], ours, truth, ref)
    assert not rep.ok and rep.bad_rows == [i]


# ---- crop_geometry

GEO = sf.geometry_cases()


def test_the_geometry_cases_are_deterministic_and_complete():
    again = sf._build_geometry_cases()
    assert len(GEO) == sf.N_GEOMETRY == 24
    assert all(np.array_equal(a['boxes'], b['boxes']) and np.array_equal(a['K'], b['K']) for a, b in zip(GEO, again))
    for kind in sf.BOX_KINDS:
        assert sum(c['kind'] == kind for c in GEO) >= 3, kind
    for up in sf.UP_KINDS:
        assert sum(c['up_kind'] == up for c in GEO) >= 4, up
    assert {c['cols'] for c in GEO} == {4, 5} and {c['dist'] for c in GEO} == {'none', 'd5', 'd12'}
    assert {c['aa'] for c in GEO} == {1, 2, 4, 8} and min(c['res'] for c in GEO) == 7 and max(c['res'] for c in GEO) == 384
    n_aug = [c['n_tta'] + len(c['hand']) for c in GEO]
    assert min(n_aug) == 1 and max(n_aug) == 6
    hand = [t for c in GEO for t in c['hand']]
    assert all(hand.count(t) >= 2 for t in sf.THRESHOLDS)
    assert sum(c['warp'] for c in GEO) >= 4
    n, h, w = sf.GEOMETRY_FRAME
    for c in GEO:
        K, box = c['K'][c['slot']], c['boxes'][c['slot']]
        assert K[0, 1] != 0 and K[0, 0] != K[1, 1] or c['up_kind'] == 'parallel'   # skew, non-square pixels
        assert (c['ids'] < n).all() and c['boxes'].shape == (2, c['cols'])
        x0, y0, x1, y1 = box[0], box[1], box[0] + box[2], box[1] + box[3]
        if c['kind'] == 'inside':
            assert x0 >= 0 and y0 >= 0 and x1 <= w and y1 <= h
        elif c['kind'] == 'partly':
            assert x0 < 0 < x1
        elif c['kind'] == 'far':
            assert x0 > w + 0.5 * w and y1 < 0
        elif c['kind'] == 'thin':
            assert box[2] == 1.0
        else:
            assert x0 < 0 and y0 < 0 and x1 > w and y1 > h


@pytest.mark.parametrize('case', GEO, ids=[f'{c["index"]}-{c["kind"]}-{c["up_kind"]}' for c in GEO])
def test_the_geometry_oracle_runs_in_float64_and_the_scales_straddle_the_thresholds(case):
    first = sf.geometry_oracle64(case, sf.geometry_augmentations(case, None))
    assert first['r_noaug'].dtype == torch.float64 and bool(torch.isfinite(first['hinv']).all())
    slot = case['slot']
    box_scale32 = np.float32(float(first['crop_scale'][0, slot]))   # stands in for the kernel's [34]
    aug = sf.geometry_augmentations(case, box_scale32)
    o = sf.geometry_oracle64(case, aug)
    assert o['hinv'].shape == (case['n_tta'] + len(case['hand']), 2, 3, 3)
    if case['up_kind'] == 'parallel':   # the fallback branch of lookat_matrix: forward x up == 0 exactly
        inp = sf.geometry_inputs(case)
        fwd = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)
        assert torch.equal(torch.linalg.cross(fwd, inp['up'][slot].double()), torch.zeros(3, dtype=torch.float64))
        assert torch.equal(o['r_noaug'][slot], torch.eye(3, dtype=torch.float64))
    else:
        assert not torch.equal(o['r_noaug'][slot], torch.eye(3, dtype=torch.float64))
    # the kernel's crop scale for a hand-made row: f32(f64(scale) * f64(box_scale32)).  An ulp of the scale is at most
    # 2^-23 of it: the quotient's rounding (1/2 ulp) and the offset (<= 2 ulp) move the product by 5 * 2^-24 of 2^-k at
    # most, its own rounding by 2^-24 more; the offsets of -2 and +2 ulp (>= 2 * 2^-24 each) outweigh the two roundings
    # (< 1.5 * 2^-24 together): they land on either side of the threshold
    for j, (k, u) in enumerate(case['hand']):
        s = np.float32(float(aug['scales'][case['n_tta'] + j]) * float(box_scale32))
        assert abs(float(s) - 2.0 ** -k) <= 6 * 2.0 ** -24 * 2.0 ** -k
        if u <= -2:
            assert float(s) < 2.0 ** -k
        if u >= 2:
            assert float(s) > 2.0 ** -k
    assert sf.exact_level(np.float32(0.5), 1) == 1 and sf.exact_level(np.nextafter(np.float32(0.5), np.float32(1)), 1) == 0
    assert sf.exact_level(np.float32(0.25), 1) == 2 and sf.exact_level(np.float32(0.126), 2) == 1
    assert sf.exact_level(np.float32(3.0), 1) == 0 and sf.exact_level(np.float32(1e-3), 4) == 2


def test_the_geometry_bounds_are_ulps():
    m = torch.tensor([[[100.0, 1e-9, 3.0], [0.0, 50.0, 1.0], [0.0, 0.0, 1.0]]], dtype=torch.float64)
    b = sf.matrix_bound(m)
    assert float(b[0, 0, 0]) == 2.0 ** -17 and float(b[0, 2, 2]) == 100 * 2.0 ** -24 and float(b[0, 0, 1]) == 100 * 2.0 ** -24
    assert float(sf.scale_bound(torch.tensor(0.75, dtype=torch.float64))) == 2 * 2.0 ** -24

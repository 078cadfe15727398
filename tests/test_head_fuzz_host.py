"""CPU: the generators and the checker of tests/head_fuzz.py (the fused head and the decode, four families of 24
seeded cases).  Nothing here launches a kernel:

  * the generators are deterministic and complete;
  * every case is accepted by the host-side argument checks of its entry point (mtr_head_plan, mtr_head_packed_bytes,
    mtr_head_fused_ws / mtr_softargmax_decode_opts with B = 0 on host pointers), and one rule broken at a time is
    refused;
  * the draw REACHES what it is there for -- every MTR_HEAD_KERNEL_* id of the family, a split launch, packed last
    blocks of 16 and of 32 positions, atoms of 1 .. 5 tiles, overflow tiles, a ragged last atom, every column-tile
    count 1 .. 8, every balanced setting -- asserted from mtr_head_row_plan and from mtr_head_plan with FORCED options
    only (the default plan may read the CU count; the forced ones are a function of shape and options);
  * the checker accepts the reference (rounded to f32, and the oracle's own f32 evaluation, on every case) and rejects
    the subtly wrong answers of head_fuzz.wrong: the seven EVERY_CASE kinds on every case they apply to, each on at
    least 8 cases of a family that has the kind at all, at least 10 bounds away; 'bias_depth' on at least half."""
import ctypes

import pytest
import torch

import head_fuzz
from head_fuzz import FAMILIES, N_CASES

MTR_E_SHAPE, MTR_E_PARAM, MTR_E_WORKSPACE = -2, -4, -5
KERNEL_IDS = {'head32': {1, 2, 3, 4}, 'head16': {10, 11, 13, 14, 15, 16, 17, 18}, 'head16rt': {12}}
FUSED = ('head32', 'head16', 'head16rt')

_store = (ctypes.c_char * (1 << 12))()
_base = (ctypes.addressof(_store) + 255) & ~255   # host pointers for the B = 0 calls: only their values are looked at


def _plan_rc(lib, c, have_workspace=True, **options):
    """(return code, mtr_head_plan_info) of mtr_head_plan on the case."""
    from metrabs_amd import _lib
    info = _lib.HeadPlanInfo()
    opts = _lib.head_options(**options)
    rc = lib.mtr_head_plan(_lib.dtype_code(c['dtype']), _lib.MTR_NHWC if c['nhwc'] else _lib.MTR_NCHW, c['B'], c['C'],
                           c['H'], c['W'], c['J'], c['D'], ctypes.byref(opts), int(have_workspace), ctypes.byref(info))
    return rc, info


def _entry_rc(lib, c, B=0):
    """The entry point on host pointers (B = 0: the argument checks, then "nothing to do")."""
    from metrabs_amd import _lib
    from metrabs_amd.config import MetrabsConfig
    hp = MetrabsConfig.from_any(head_fuzz.head_config(c).as_dict()).head_params()
    layout = _lib.MTR_NHWC if c['nhwc'] else _lib.MTR_NCHW
    x, pk, c2, c3 = (ctypes.c_void_p(_base + 256 * k) for k in range(4))
    if c['family'] == 'decode':
        return lib.mtr_softargmax_decode_opts(x, _lib.dtype_code(c['dtype']), layout, B, c['J'], c['D'], c['H'], c['W'],
                                              ctypes.byref(hp), 0, c2, c3, None)
    opts = _lib.head_options()
    return lib.mtr_head_fused_ws(x, _lib.dtype_code(c['dtype']), layout, B, c['C'], c['H'], c['W'], pk, c['J'], c['D'],
                                 ctypes.byref(hp), ctypes.byref(opts), None, 0, c2, c3, None)


@pytest.mark.parametrize('family', FAMILIES)
def test_generators_are_deterministic_and_complete(family):
    a, b = head_fuzz.build_cases(family), head_fuzz.build_cases(family)
    assert len(a) == N_CASES and a == b == head_fuzz.cases(family)
    assert len({head_fuzz.case_id(c) for c in a}) == N_CASES
    for c in a:     # the inputs too
        x, y = head_fuzz.inputs(c), head_fuzz.inputs(c)
        assert all(torch.equal(x[k], y[k]) for k in x)


@pytest.mark.parametrize('family', FAMILIES)
def test_every_case_is_accepted(family, hip_lib):
    from metrabs_amd import _lib, kernels
    for c in head_fuzz.cases(family):
        B, C, J, D, H, W = (c[k] for k in 'BCJDHW')
        assert min(B, J, D, H, W) >= 1 and c['proc_side'] >= 1, c
        assert _entry_rc(hip_lib, c) == 0, head_fuzz.case_id(c)
        if family == 'decode':
            continue
        # the family's rules, stated once more on the drawn case
        assert (H * W) % 4 == 0 and D <= 80 and (not c['nhwc'] or C % 4 == 0)
        if family == 'head16':
            assert C % 8 == 0 and 1 + D <= 64 and H * W <= 256
        if family == 'head16rt':
            assert C % 64 == 0 and (1 + D > 64 or H * W > 256)
        assert kernels.head_fused_supported(C, J, D, H, W, c['nhwc'], c['dtype'])
        assert _plan_rc(hip_lib, c)[0] == 0, head_fuzz.case_id(c)
        needs_ws = family == 'head16rt' and not c['nhwc']
        assert _plan_rc(hip_lib, c, have_workspace=False)[0] == (MTR_E_WORKSPACE if needs_ws else 0), head_fuzz.case_id(c)
        assert hip_lib.mtr_head_packed_bytes(C, J, D, _lib.dtype_code(c['dtype'])) > 0
        ws = hip_lib.mtr_head_workspace_bytes(_lib.dtype_code(c['dtype']), _lib.MTR_NHWC if c['nhwc'] else _lib.MTR_NCHW,
                                              B, C, H, W, J, D)
        assert not needs_ws or ws > 0
    print(f'{family}: {N_CASES} accepted cases')


@pytest.mark.parametrize('family', FAMILIES)
def test_one_rule_broken_is_refused(family, hip_lib):
    from metrabs_amd import _lib
    cs = head_fuzz.cases(family)
    base = cs[0]
    assert _entry_rc(hip_lib, base) == 0
    assert _entry_rc(hip_lib, dict(base, proc_side=0)) == MTR_E_PARAM
    if family == 'decode':
        assert _entry_rc(hip_lib, dict(base, D=0)) == MTR_E_SHAPE
        return
    H, W = base['H'], base['W']
    odd = dict(base, H=H + 1 if H % 2 == 0 else H, W=W + 1 if W % 2 == 0 else W)     # both odd: H*W % 4 != 0
    assert (odd['H'] * odd['W']) % 4 != 0
    assert _entry_rc(hip_lib, odd) == MTR_E_SHAPE and _plan_rc(hip_lib, odd)[0] == MTR_E_SHAPE
    deep = dict(base, D=81)
    assert _entry_rc(hip_lib, deep) == MTR_E_SHAPE and _plan_rc(hip_lib, deep)[0] == MTR_E_SHAPE
    nhwc = next(c for c in cs if c['nhwc'])
    off4 = dict(nhwc, C=nhwc['C'] + 2)
    assert _entry_rc(hip_lib, off4) == MTR_E_SHAPE and _plan_rc(hip_lib, off4)[0] == MTR_E_SHAPE
    if family != 'head32':
        off8 = dict(next(c for c in cs if not c['nhwc']), C=base['C'] + 4)
        assert hip_lib.mtr_head_packed_bytes(off8['C'], off8['J'], off8['D'], _lib.dtype_code(off8['dtype'])) == 0
        assert _entry_rc(hip_lib, off8) == MTR_E_SHAPE


def _row_plan(lib, J, D):
    n_tiles, per_atom = ctypes.c_int32(), ctypes.c_int32()
    assert lib.mtr_head_row_plan(J, D, ctypes.byref(n_tiles), ctypes.byref(per_atom), None, 0) == 0
    rows = (ctypes.c_int32 * (n_tiles.value * 16))()
    assert lib.mtr_head_row_plan(J, D, ctypes.byref(n_tiles), ctypes.byref(per_atom), rows, len(rows)) == 0
    rows = list(rows)
    assert sorted(r for r in rows if r >= 0) == list(range(J * (1 + D))), 'every channel in exactly one packed row'
    tiles = [rows[16 * t:16 * t + 16] for t in range(n_tiles.value)]
    overflow = sum(1 for t in tiles if all(r < J for r in t) and any(r >= 0 for r in t))   # 2D rows only
    a = per_atom.value
    n_atoms = (n_tiles.value - overflow) // a
    depth_rows = lambda k: sum(1 for t in tiles[k * a:(k + 1) * a] for r in t if r >= J)
    ragged = n_atoms >= 2 and depth_rows(n_atoms - 1) < depth_rows(0)
    return a, overflow, ragged


# every dispatch choice given: the plan is a function of shape and options
_FORCED32 = ([dict(rt_tiles=t, rt_loader=ld, rt_split=1, rt_column_blocks=1, rt_k_groups=1) for ld in (1, 2) for t in range(1, 6)]
             + [dict(rt_tiles=t, rt_loader=1, rt_split=1, rt_column_blocks=1, rt_k_groups=2) for t in (1, 2, 3)]
             + [dict(rt_tiles=1, rt_loader=1, rt_split=1, rt_column_blocks=n, rt_k_groups=1) for n in (2, 3, 4)]
             + [dict(rt_tiles=t, rt_loader=1, rt_split=2, rt_column_blocks=1, rt_k_groups=1) for t in (1, 3)])
_FORCED16 = [dict(dma_staging=s, groups_per_workgroup=g) for s in range(8) for g in (1, 2, 3, 4)]
_FORCED16RT = [dict(rt_tiles=t, rt_split=s) for t in range(1, 6) for s in (1, 2)]


@pytest.mark.parametrize('family', FUSED)
def test_the_draw_reaches_every_kernel_and_tiling(family, hip_lib):
    cs = head_fuzz.cases(family)
    forced = {'head32': _FORCED32, 'head16': _FORCED16, 'head16rt': _FORCED16RT}[family]
    kernels_hit, split, packed, np_blocks, tiles_per_wg = set(), False, set(), set(), set()
    for c in cs:
        for opts in forced:
            rc, info = _plan_rc(hip_lib, c, **opts)
            assert rc == 0, (head_fuzz.case_id(c), opts)
            kernels_hit.add(info.kernel)
            tiles_per_wg.add(info.tiles_per_workgroup)
            np_blocks.add(info.column_blocks)
            if info.split_column_blocks >= 2:
                split = True
                assert info.split_column_blocks == head_fuzz.n_column_blocks(c)
                tail = (c['H'] * c['W']) % 64
                if family == 'head32' and tail in (16, 32):   # rt_dispatch: those of 4 / 2 consecutive crops share a workgroup
                    packed.add((tail, c['B'] % 4))
    assert kernels_hit == KERNEL_IDS[family], kernels_hit
    print(f'{family}: kernels {sorted(kernels_hit)}, tiles per workgroup {sorted(tiles_per_wg)}, column blocks '
          f'{sorted(np_blocks)}, split {split}, packed last blocks (positions, B % 4) {sorted(packed)}')
    if family != 'head16':
        assert split
        plans = [_row_plan(hip_lib, c['J'], c['D']) for c in cs]
        assert {p[0] for p in plans} == {1, 2, 3, 4, 5}, 'atoms of 1 .. 5 tiles'
        assert any(p[1] for p in plans), 'overflow tiles of 2D rows'
        assert any(p[2] for p in plans), 'a ragged last atom'
        assert max(head_fuzz.n_column_blocks(c) for c in cs) >= 5, 'a workgroup tile of up to four column blocks wraps'
    if family == 'head32':
        assert {t for t, _ in packed} == {16, 32}, packed
        assert any(b for _, b in packed), 'a packed last block at B % 4 != 0'
        assert np_blocks >= {1, 2, 3, 4} and tiles_per_wg >= {1, 2, 3, 4, 5}
        assert {c['C'] % 64 == 0 for c in cs} == {True, False} and {c['C'] % 32 == 0 for c in cs} == {True, False}
    if family == 'head16':
        assert {(c['H'] * c['W'] + 31) // 32 for c in cs} == set(range(1, 9)), 'every column-tile count 1 .. 8'
        assert any(c['C'] == head_fuzz.C_RESIDENT and c['B'] == 2 for c in cs)
        assert {c['C'] % 64 == 0 for c in cs} == {True, False} and any(c['C'] < 64 for c in cs)


@pytest.mark.parametrize('family', FAMILIES)
def test_the_draw_reaches_every_balanced_setting(family):
    cs = head_fuzz.cases(family)
    reach = lambda key, among=None: {c[key] for c in cs if among is None or c['kind'] == among}
    assert reach('stride') == set(head_fuzz.STRIDES)
    assert reach('proc_kind') == set(head_fuzz.PROC_KINDS)
    assert {(c['centered'], c['legacy']) for c in cs} == set(head_fuzz.FLAGS)
    assert reach('box') == set(head_fuzz.BOXES)
    assert reach('kind') == set(head_fuzz.KINDS) and reach('nhwc') == {False, True}
    assert reach('B') == set(head_fuzz.B_VALUES) and reach('J') >= {1, 2, 3, 5}
    assert reach('rotation', 'spike') == {0, 1, 2, 3} and reach('amp', 'spike') == set(head_fuzz.SPIKES)
    assert reach('larger_first', 'two_peaks') == {True, False} and reach('level_3d', 'level') == {True, False}
    assert reach('dtype') == ({torch.float32} if family == 'head32' else {torch.float16, torch.bfloat16} if
                              family != 'decode' else {torch.float32, torch.float16, torch.bfloat16})
    # the shipped combinations, and a proc_side whose last pixel is no stride centre
    s256, l384 = cs[0], cs[1]
    assert (s256['proc_side'], s256['stride'], s256['centered'], s256['legacy'], s256['box']) == (256, 32, False, True, 2200.0)
    assert (l384['proc_side'], l384['stride'], l384['centered'], l384['legacy'], l384['box']) == (384, 32, True, False, 2200.0)
    assert any((c['proc_side'] - 1) % c['stride'] != c['stride'] - 1 for c in cs)
    assert any(c['H'] != c['W'] for c in cs) and any(c['H'] == c['W'] for c in cs)
    if family == 'decode':
        assert any(c['W'] % 4 != 0 for c in cs) and any((c['H'] * c['W']) % 2 == 1 for c in cs)
        assert any(c['H'] == 1 for c in cs) and any(c['W'] == 1 for c in cs)
    # two peaks in different column blocks, and for D > 16 in different tiles of the atom
    assert any(c['kind'] == 'two_peaks' and head_fuzz.n_column_blocks(c) >= 2 for c in cs)


@pytest.mark.parametrize('family', FAMILIES)
def test_the_checker_accepts_the_reference_and_rejects_wrong_ones(family):
    cs = head_fuzz.cases(family)
    table = {k: [0, 0] for k in head_fuzz.WRONG}     # kind -> [rejected, applicable]
    nearest = {k: float('inf') for k in head_fuzz.WRONG}
    worst32 = 0.0
    for c in cs:
        inp, ref, bnd = head_fuzz.truth(c)
        assert all(bool((b >= 0).all()) and bool(torch.isfinite(b).all()) for b in bnd), head_fuzz.case_id(c)
        assert head_fuzz.ratio([r.float() for r in ref], ref, bnd) <= 1.0, head_fuzz.case_id(c)
        r32 = head_fuzz.ratio(head_fuzz.oracle32(c, inp), ref, bnd)
        assert r32 <= 1.0, (head_fuzz.case_id(c), r32)
        worst32 = max(worst32, r32)
        nan = [r.float().clone() for r in ref]
        nan[1][-1, -1, -1] = float('nan')
        assert head_fuzz.ratio(nan, ref, bnd) == float('inf')
        for kind in head_fuzz.WRONG:
            if not head_fuzz.wrong_applies(kind, c):
                continue
            bad = [w.float() for w in head_fuzz.wrong(kind, c, inp)]     # as a kernel would return it
            d = head_fuzz.ratio(bad, ref, bnd)
            table[kind][1] += 1
            if d > 1.0:
                table[kind][0] += 1
                nearest[kind] = min(nearest[kind], d)
            else:   # accepted only where it lies within the bound plus its own rounding of the right answer
                exact = head_fuzz.wrong(kind, c, inp)
                assert all(bool(((w - r).abs() <= b + head_fuzz.U * w.abs()).all()) for w, r, b in zip(exact, ref, bnd))
                assert kind not in head_fuzz.EVERY_CASE, (head_fuzz.case_id(c), kind, d)
    print(f'{family}: the f32 oracle inside the bound on all {len(cs)} cases, at most {worst32:.2f} of it')
    for kind, (rejected, applicable) in table.items():
        print(f'{family}: {kind:14s} rejected {rejected} / {applicable} applicable, nearest {nearest[kind]:.1f} bounds')
        if applicable == 0:     # the family does not have the kind (head_fuzz.wrong_applies)
            assert family == 'decode' and kind in ('last_channel', 'bias_depth')
        elif kind in head_fuzz.EVERY_CASE:
            assert rejected == applicable >= 8, (kind, rejected, applicable)
            assert nearest[kind] >= 10.0, (kind, nearest[kind])
        else:
            assert 2 * rejected >= applicable, (kind, rejected, applicable)

"""GPU: the crop sampler (K6: pyramid, crop_geometry, the two warp kernels, the antialias > 4 shrink) on the seeded fuzz
of tests/sampler_fuzz.py, against the row's own formula in float64.

Bounds.  Crops: per frame set and per kernel (row-walking; per-tap / antialias 4), max and mean of |ours - fp64| in
linear light within 4x the reference's own float32 distance to the same fp64 values, measured in the same call, plus
8 * 2^-24 (sampler_fuzz.check).  The 4x margin is the project's rule for this sampler (docstring of
tests/test_gpu_sampler.py), not a measurement of this module; what was measured is below.  Geometry: f32 ulps, derived
next to sampler_fuzz.matrix_bound / scale_bound.

Measured on an MI355X (the [parity] lines of this module), ours / reference for max and mean, then the reference's own
floor (max, mean) in linear light:

    frame set   kernel   max   mean    floor max  floor mean
    2x120x160   rows     0.64  0.69    3.33e-06   4.96e-08
    2x120x160   taps     1.34  1.00    2.07e-06   4.66e-08
    1x64x200    rows     1.13  0.94    1.09e-05   1.99e-07
    1x64x200    taps     0.87  1.04    3.28e-06   7.21e-08
    3x97x131    rows     1.25  1.09    8.16e-06   8.61e-08
    3x97x131    taps     0.51  0.71    1.77e-06   6.10e-08
    2x75x99     rows     1.00  0.87    3.51e-06   8.28e-08
    2x75x99     taps     0.46  0.86    3.51e-06   7.09e-08
    2x64x66     rows     0.80  0.81    4.84e-06   5.89e-08
    2x64x66     taps     0.68  0.99    2.12e-07   1.78e-08
    2x51x101    rows     0.93  0.95    6.57e-06   5.85e-08
    2x51x101    taps     0.86  0.94    8.77e-07   2.36e-08
    3x88x45     rows     0.54  0.80    8.52e-06   8.40e-08
    3x88x45     taps     0.53  0.67    1.59e-06   3.91e-08
    2x9x37      rows     1.11  1.00    1.53e-06   5.96e-08
    2x9x37      taps     1.23  1.01    1.85e-07   6.99e-09
    1x43x10     rows     0.60  0.84    3.94e-06   5.94e-08
    1x43x10     taps     1.38  1.15    4.89e-07   1.99e-08
    2x6x29      taps     0.93  1.14    1.30e-06   2.50e-08
    3x23x5      taps     0.47  0.80    3.33e-06   4.46e-08
    1x3x18      taps     1.15  0.93    7.37e-07   1.69e-08
    2x14x2      taps     0.97  0.86    6.50e-07   1.57e-08

The rows crop_geometry wrote, through the sampler (nine of the 24 geometry cases, row-walking kernel): max 0.66 .. 1.49,
mean 0.76 .. 1.61 of a floor of 3.3e-07 .. 4.5e-06 max / 4.2e-08 .. 2.5e-07 mean.  No pool is beyond 1.61x of the
reference's own distance to fp64 (the frame-set pools: 1.38x); the fuzz found no fault in the kernels.  Level 0 is NOT
within one f32 ulp of the fp64 (v / 255) ** 2.2 per element (up to 2.8 ulp, at v = 3): the table holds the reference's
f32 expression on its f32-rounded operands, evaluated exactly -- see _pyramids.
"""
import numpy as np
import pytest
import torch

import sampler_fuzz as sf
from conv_fuzz import SENTINEL, bands_intact, guarded_out
from oracle import cases

pytestmark = pytest.mark.gpu

SETS = sf.frame_sets()
GEO = sf.geometry_cases()
DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _guarded_crops(n, res, dtype, channels_last, device='cuda'):
    """(buffer, out): a sentinel-filled crop tensor [n,3,res,res] in the layout asked for, inside sentinel bands."""
    if channels_last:
        big, mem = guarded_out((n, res, res, 3), dtype, device)
        return big, mem.permute(0, 3, 1, 2)
    return guarded_out((n, 3, res, res), dtype, device)


def _warp_guarded(kernels, pyr, wp, res, aa, dtype=torch.float32, channels_last=False):
    big, out = _guarded_crops(wp.shape[0], res, dtype, channels_last)
    got = kernels.warp_crops(pyr, wp, res, aa, out_dtype=dtype, channels_last=channels_last, out=out)
    assert got is out and bands_intact(big), 'the sampler wrote outside its crops'
    assert bool((out != SENTINEL).all()), 'the sampler left crop elements unwritten'
    return out


def _pyramids(kernels, frames_u8):
    """The materialised pyramid and its CPU copy, the planar-u8 and the interleaved-u8 ones -- all checked here:
    level 0 within 2.4e-7 of the fp64 (v / 255) ** 2.2 (the existing rule of test_pyramid_vs_oracle: 2 ulp at 1) and,
    per element, within half an f32 ulp of what the table is: the reference's f32 expression (images.float() / 255) ** 2.2
    on its f32 operands f32(v / 255) and f32(2.2), evaluated in fp64 and rounded once (common.h).  Two operand roundings
    set it apart from the fp64 value of the unrounded v / 255 and 2.2: the base's (up to 2^-24 relative, times the
    exponent) and the exponent's (f32(2.2) - 2.2 = 4.8e-8, times |ln(base)|, which grows on dark values) -- up to 2.8 f32
    ulp of the value, at v = 3, and 4.2e-8 absolute at most; levels 1 / 2
    bit-equal to F.avg_pool2d of THAT level 0, and the three other ways to the same levels bit-equal to it."""
    planar = frames_u8.cuda()
    inter = planar.contiguous(memory_format=torch.channels_last)
    mat = kernels.build_pyramid(planar, materialize_level0=True)
    levels = [l.cpu() for l in mat.levels]
    want0 = (frames_u8.double() / 255) ** 2.2
    assert float((levels[0].double() - want0).abs().max()) <= 2.4e-7
    table = (frames_u8.float() / 255).double() ** float(np.float32(2.2))
    assert bool(((levels[0].double() - table).abs() <= 0.5 * cases.f32_ulp_at(table)).all())
    pooled = sf.cpu_pyramid(levels[0])
    for lvl in (1, 2):
        assert levels[lvl].shape == pooled[lvl].shape and torch.equal(levels[lvl], pooled[lvl]), lvl
    p_planar, p_inter, p_float = kernels.build_pyramid(planar), kernels.build_pyramid(inter), \
        kernels.pyramid_from_level0(mat.levels[0])
    assert p_planar.levels[0] is None and p_inter.levels[0] is None and not p_planar.hwc
    assert p_inter.hwc == kernels.frames_are_interleaved(inter)
    for other in (p_planar, p_inter, p_float):
        for lvl in (1, 2):
            assert torch.equal(other.levels[lvl], mat.levels[lvl]), lvl
    assert torch.equal(p_planar.lut, p_inter.lut)
    return mat, levels, p_planar, p_inter


@pytest.mark.parametrize('fs', SETS, ids=[fs['name'] for fs in SETS])
def test_sampler_fuzz_frame_set(fs, hip_lib):
    from metrabs_amd import kernels
    mat, levels, p_planar, p_inter = _pyramids(kernels, sf.frames_of(fs))
    ours = [None] * len(fs['rows'])
    for g in range(len(fs['groups'])):
        idx, wp, res, aa = sf.group_rows(fs, g)
        wp = wp.cuda()
        base = _warp_guarded(kernels, mat, wp, res, aa)
        for pyr in (mat, p_planar, p_inter):
            for dtype in DTYPES:
                for cl in (False, True):
                    if pyr is mat and dtype == torch.float32 and not cl:
                        continue
                    got = _warp_guarded(kernels, pyr, wp, res, aa, dtype, cl)
                    assert got.is_contiguous(memory_format=torch.channels_last) or not cl or got.shape[0] == 0
                    assert torch.equal(got, base.to(dtype)), (fs['name'], g, dtype, cl, pyr.hwc)
        for j, i in enumerate(idx):
            ours[i] = base[j].cpu()
    with torch.inference_mode():
        truth = [sf.yardstick(levels, r) for r in fs['rows']]
        ref = [sf.reference32(levels, r) for r in fs['rows']]
    rep = sf.check(fs['name'], fs['rows'], ours, truth, ref)
    print('\n'.join(rep.lines))
    assert rep.ok, rep.failures


# ---- crop_geometry

_GEO_PYRAMIDS = {}


def _geometry_pyramids(kernels):
    if not _GEO_PYRAMIDS:
        frames = cases.synth_images(*sf.GEOMETRY_FRAME, sf.GEOMETRY_SEED)
        _GEO_PYRAMIDS['p'] = _pyramids(kernels, frames)
    return _GEO_PYRAMIDS['p']


@pytest.mark.parametrize('case', GEO, ids=[f'{c["index"]}-{c["kind"]}-{c["up_kind"]}' for c in GEO])
def test_crop_geometry_fuzz(case, hip_lib):
    from metrabs_amd import kernels
    inp = {k: v.cuda() for k, v in sf.geometry_inputs(case).items()}
    res, aa, slot = case['res'], case['aa'], case['slot']

    def run(aug):
        return kernels.crop_geometry(inp['boxes'], inp['K'], inp['dist12'], inp['up'], inp['ids'], aug['rotflipmat'].cuda(),
                                     aug['scales'].cuda(), aug['gammas'].cuda(), res, aa)

    _, _, wp1 = run(sf.geometry_augmentations(case, None))
    box_scale = float(wp1[slot, 34])                  # augmentation 0 has a scale of 1: [34] is f32(box_scale)
    aug = sf.geometry_augmentations(case, box_scale)
    new_k, rot, wp = run(aug)
    A = aug['scales'].shape[0]
    assert new_k.shape == rot.shape == (A, 2, 3, 3) and wp.shape == (A * 2, 36)
    new_k, rot, wp = new_k.cpu().double(), rot.cpu().double(), wp.cpu()
    rows = wp.reshape(A, 2, 36)
    s32 = rows[..., 34]
    o = sf.geometry_oracle64(case, aug, s32)
    # crop scale: rounded twice (sampler_fuzz.scale_bound)
    assert bool(((s32.double() - o['crop_scale']).abs() <= sf.scale_bound(o['crop_scale'])).all()), \
        (s32.double() - o['crop_scale']).abs() / sf.scale_bound(o['crop_scale'])
    assert abs(float(o['box_scales'][slot]) - box_scale) <= float(sf.scale_bound(o['box_scales'][slot])) / 2
    # the matrices, recomputed in fp64 from the row's own scale: rounded once (sampler_fuzz.matrix_bound)
    for name, got, want in (('new_k', new_k, o['new_k']), ('rot', rot, o['rot']),
                            ('Hinv', rows[..., 0:9].reshape(A, 2, 3, 3).double(), o['hinv']),
                            ('K_level', rows[..., 9:18].reshape(A, 2, 3, 3).double(), o['k_level'])):
        over = (got - want).abs() / sf.matrix_bound(want)
        assert float(over.max()) <= 1.0, (name, float(over.max()))
    # exact fields
    assert torch.equal(rows[..., 31].long(), o['level']), (rows[..., 31], o['level'], s32)
    assert torch.equal(rows[..., 18:30], inp['dist12'].cpu()[None].expand(A, 2, 12))
    assert torch.equal(rows[..., 30], (inp['dist12'].cpu() != 0).any(dim=1).float()[None].expand(A, 2))
    assert torch.equal(rows[..., 32], inp['ids'].cpu().float()[None].expand(A, 2))
    assert np.array_equal(rows[..., 33].numpy(), np.repeat(o['gexp'][:, None], 2, axis=1))
    assert bool((rows[..., 35] == 0).all())
    if not case['warp']:
        return
    # the fields one kernel writes are the fields the other reads: these rows through the sampler and the checker
    mat, levels, p_planar, _ = _geometry_pyramids(kernels)
    n, h, w = sf.GEOMETRY_FRAME
    warp_rows = [dict(wp=r.numpy(), res=res, aa=aa, level=int(r[31]), img=int(r[32]), gexp=float(r[33]), cls='geometry',
                      kernel=sf.kernel_pool(h, w, aa)) for r in wp]
    for r in warp_rows:
        _, _, oz, den = sf.positions(r['wp'], res, aa)
        assert float(oz.min()) > 0 and float(den.min()) > 0.5 and r['img'] < n
    base = _warp_guarded(kernels, mat, wp.cuda(), res, aa)
    assert torch.equal(_warp_guarded(kernels, p_planar, wp.cuda(), res, aa), base)
    with torch.inference_mode():
        truth = [sf.yardstick(levels, r) for r in warp_rows]
        ref = [sf.reference32(levels, r) for r in warp_rows]
    rep = sf.check(f'geometry case {case["index"]}', warp_rows, list(base.cpu()), truth, ref)
    print('\n'.join(rep.lines))
    assert rep.ok, rep.failures


# ---- antialias > 4

def _antialias_rows(kernels, res, aa):
    n, h, w = sf.GEOMETRY_FRAME
    tta = sf.cpu_ref.tta_params(5)
    boxes = torch.tensor([[20.0, 10.0, 60.0, 70.0]])
    _, _, wp = kernels.crop_geometry(
        boxes.cuda(), cases.intrinsics_for(h, w, 55.0, 3)[None].cuda(), torch.zeros(1, 12).cuda(),
        torch.tensor([[0.0, -1.0, 0.0]]).cuda(), torch.tensor([1]).cuda(), tta['rotflipmat'].cuda(),
        tta['scales'].cuda(), tta['gammas'].cuda(), res, aa)
    wp[0, 33] = 1.0   # one crop without a gamma step: its shrink is aten's filter bit for bit
    return wp


def test_antialias_above_4_runs_in_chunks_with_the_single_chunk_bits(hip_lib, monkeypatch):
    import torch.nn.functional as F
    from metrabs_amd import kernels
    res, aa = 8, 6
    mat, _, _, p_inter = _geometry_pyramids(kernels)
    wp = _antialias_rows(kernels, res, aa)
    n = wp.shape[0]
    assert n == 5
    whole = {}
    for dtype in DTYPES:
        for cl in (False, True):
            whole[dtype, cl] = kernels.warp_crops(mat, wp, res, aa, out_dtype=dtype, channels_last=cl)
    # the single-chunk f32 result against the oracle's filter on the same res*aa crops -- OUR crops, sampled here: this
    # checks the shrink and the chunking, not the large crops themselves (the sampler is fuzzed above) -- with the bound of
    # test_antialias_above_4_shrink_is_atens_filter (bit-equal without a gamma step, 2e-6 with the device pow)
    wp_lin = wp.clone()
    wp_lin[:, 33] = 1.0
    big = kernels.warp_crops(mat, wp_lin, res * aa, 1).cpu()
    want = F.interpolate(big, size=[res, res], mode='bilinear', align_corners=False, antialias=True)
    got = whole[torch.float32, False].cpu()
    assert torch.equal(got[0], want[0])
    gexp = wp[:, 33].cpu().reshape(n, 1, 1, 1)
    assert float((got - want ** gexp).abs().max()) <= 2e-6
    assert torch.equal(whole[torch.float32, True], whole[torch.float32, False])
    # ... and in three chunks (2 + 2 + 1 crops), every layout and dtype, into guarded buffers
    per = 3 * (res * aa) ** 2 * 4
    monkeypatch.setattr(kernels, 'MAX_BIG_CROP_BYTES', 2 * per + per // 2)
    inner = kernels.warp_crops
    chunks = []

    def counting(pyramid, warp_params, r, antialias=1, *args, **kw):
        if antialias == 1 and r == res * aa:
            chunks.append(warp_params.shape[0])
        return inner(pyramid, warp_params, r, antialias, *args, **kw)

    monkeypatch.setattr(kernels, 'warp_crops', counting)
    for pyr in (mat, p_inter):
        for dtype in DTYPES:
            for cl in (False, True):
                del chunks[:]
                got = _warp_guarded(kernels, pyr, wp, res, aa, dtype, cl)
                assert chunks == [2, 2, 1], chunks
                assert torch.equal(got, whole[dtype, cl]), (dtype, cl, pyr.hwc)


# ---- refusals

def test_warp_crops_refuses_rows_and_outputs_it_would_misread(hip_lib):
    from metrabs_amd import kernels
    fs = SETS[0]
    mat = kernels.build_pyramid(sf.frames_of(fs).cuda(), materialize_level0=True)
    res, n = 18, 3
    wp = torch.from_numpy(np.stack([r['wp'] for r in fs['rows'] if not r['persp']][:n])).cuda()
    good = kernels.warp_crops(mat, wp, res, 1)
    wide = torch.zeros(n, 72, device='cuda')
    wide[:, :36] = wp
    bad_rows = {'non-contiguous': wide[:, :36], 'float64': wp.double(), 'on the CPU': wp.cpu(),
                '35 columns': wp[:, :35].contiguous(), 'one dimension': wp.reshape(-1)}
    for what, rows in bad_rows.items():
        for aa in (1, 6):
            big, out = _guarded_crops(n, res, torch.float32, False)
            with pytest.raises(ValueError):
                kernels.warp_crops(mat, rows, res, aa, out=out)
            assert bool((big == SENTINEL).all()), what
    bad_out = {'one crop short': (lambda: _guarded_crops(n - 1, res, torch.float32, False), False, torch.float32),
               'another resolution': (lambda: _guarded_crops(n, res + 2, torch.float32, False), False, torch.float32),
               'float16 for float32': (lambda: _guarded_crops(n, res, torch.float16, False), False, torch.float32),
               'float32 for bfloat16': (lambda: _guarded_crops(n, res, torch.float32, False), False, torch.bfloat16),
               'planes for channels_last': (lambda: _guarded_crops(n, res, torch.float32, False), True, torch.float32),
               'channels_last for planes': (lambda: _guarded_crops(n, res, torch.float32, True), False, torch.float32)}
    for what, (make, cl, dtype) in bad_out.items():
        for aa in (1, 6):
            big, out = make()
            with pytest.raises(ValueError):
                kernels.warp_crops(mat, wp, res, aa, out_dtype=dtype, channels_last=cl, out=out)
            assert bool((big == SENTINEL).all()), what
    # what is accepted still gives the same bits
    assert torch.equal(_warp_guarded(kernels, mat, wp, res, 1), good)

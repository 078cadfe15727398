"""Seeded fuzz of the crop sampler (K6, csrc/warp.hip) over the frames it accepts: a helper of
tests/test_sampler_fuzz_host.py (CPU) and tests/test_gpu_sampler_fuzz.py (GPU), no test module itself.

  * frame_sets(): FRAME_SETS x 17 .. 23 warp rows each, packed BY HAND in the 36-float layout of include/metrabs_hip.h
    from random.Random(a fixed seed) -- the level is chosen, not derived from a scale, and every row is PLACED in a class
    (inside, over a border, over a corner, outside, magnified, minified, rotated, flipped, perspective).  Every row lies
    in the sampler's domain by construction (oz > 0, distortion denominator > 0.5, image id < N, no empty level):
    nothing is drawn and rejected; _assert_domain_and_class states it in fp64.
  * yardstick(): the row's own formula in float64 with direct pixel coordinates and zero padding -- homography,
    projection, distortion, K of the level, bilinear taps, mean over the aa^2 sub-samples: what the kernel's comments say
    it computes.  It equals cpu_ref.warp_single_image(eval_dtype=float64) to 1e-12 wherever every side of the level is
    at least 2 (tests/test_sampler_fuzz_host.py).  Where a side is 1 the reference divides by zero (grid_sample
    normalises by size - 1 and returns NaN): THERE THE DIRECT FORMULA IS THE SPECIFICATION -- a tap outside
    [0, W-1] x [0, H-1] contributes zero -- and reference32() evaluates the same direct formula in float32.
  * check(): ours against the yardstick in linear light, per frame set and per kernel (launch_warp's rule restated in
    uses_rows_kernel), max and mean within 4x the reference's own f32 floor measured in the same call + 8 * 2^-24.
    4x the reference's floor is the project's rule (docstring of tests/test_gpu_sampler.py); 8 * 2^-24 is about eight
    f32 roundings on values of at most 1, for pools where the reference is nearly exact.  No other tolerance is defined.
  * wrong(): subtly wrong fp64 evaluations for the checker's self-test.
  * geometry_cases(): 24 draws of (box, camera) with 1 .. 6 augmentations for crop_geometry, with the oracle's formulas
    on float64 tensors (geometry_oracle64) and the bounds in f32 ulps (matrix_bound, scale_bound).
"""
import math
import random

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cases, cpu_ref

SEED = 60606
# (N, H, W): sides <= 200
FRAME_SETS = [
    (2, 120, 160),   # multiples of 8: the wide pyramid kernel; W % 4 == 0
    (1, 64, 200),    # multiples of 8; W % 4 == 0
    (3, 97, 131),    # odd H; W % 4 == 3
    (2, 75, 99),     # odd H; W % 4 == 3
    (2, 64, 66),     # H a multiple of 8, W not; W % 4 == 2
    (2, 51, 101),    # odd H; W % 4 == 1
    (3, 88, 45),     # W % 4 == 1, portrait
    (2, 9, 37),      # min side 8..11: level 2 has exactly two rows (the smallest the row-walking kernel takes); W % 4 == 1
    (1, 43, 10),     # min side 8..11: level 2 has exactly two columns; W % 4 == 2
    (2, 6, 29),      # min side 4..7: level 2 has one row -> the per-tap kernel for every level
    (3, 23, 5),      # min side 4..7: level 2 has one column
    (1, 3, 18),      # a side of 3: level 1 has one row, level 2 is empty
    (2, 14, 2),      # a side of 2: level 1 has one column, level 2 is empty
]
RES = (7, 18, 20, 30, 32, 33, 40)
AAS = (1, 2, 4)
BORDERS = ('left', 'right', 'top', 'bottom')
CORNERS = ('tl', 'tr', 'bl', 'br')
CLASSES = ('inside',) + BORDERS + CORNERS + ('last_br', 'outside', 'magnified', 'minified', 'rotated', 'flipped',
                                             'perspective')
ABS_FLOOR = 8 * 2.0 ** -24
MARGIN = 4.0
F64 = torch.float64
_TTA_GAMMAS = (0.6, 0.7, 0.8, 0.9)   # cpu_ref.tta_params(5)['gammas'] without the 1.0


def level_dims(h, w):
    return [(h, w), (h // 2, w // 2), (h // 2 // 2, w // 2 // 2)]


def uses_rows_kernel(h, w, aa):
    """launch_warp (csrc/warp.hip): warp_rows_kernel unless antialias is 4 or ANY of the three levels has fewer than two
    rows or columns (an empty level included); warp_crops_kernel -- per-tap on the degenerate levels -- otherwise."""
    return aa <= 2 and all(lh >= 2 and lw >= 2 for lh, lw in level_dims(h, w))


def kernel_pool(h, w, aa):
    return 'rows' if uses_rows_kernel(h, w, aa) else 'taps'


def tta_exponent(i):
    return float(np.float32(_TTA_GAMMAS[i % len(_TTA_GAMMAS)]) / np.float32(2.2))


# ---- the rows

def _rot(theta):
    return np.array([[math.cos(theta), -math.sin(theta)], [math.sin(theta), math.cos(theta)]])


def _distortion(rng, kind, signs_drawn=True):
    base = {'none': (), 'd5': cases.DISTORTION_5, 'd12': cases.DISTORTION_12}[kind]
    d = np.zeros(12)
    for i, v in enumerate(base):
        sign = rng.choice((-1.0, 1.0)) if signs_drawn else 1.0
        d[i] = sign * v * rng.uniform(0.5, 1.0)
    return d


def _make_row(rng, dims, full_side, level, cls, res, aa, img, gexp, dist_kind, twist):
    hl, wl = dims[level]
    rt = res * aa
    span = max(min(hl, wl) - 1, 0)
    spanx, spany = wl - 1, hl - 1
    wide = max(0.3 * span, 2.5)
    jit = lambda a: rng.uniform(-a, a)
    cxm, cym = spanx / 2, spany / 2
    theta, flip, persp = math.radians(jit(8.0)), False, (0.0, 0.0)
    place = 'br' if cls == 'last_br' else cls
    if place == 'outside':
        side = rng.choice(BORDERS)
        e = max(0.25 * span, 2.0)
        far = 1.6 * e + 3.0
        c = {'left': (-1 - far, cym), 'right': (wl + far, cym), 'top': (cxm, -1 - far), 'bottom': (cxm, hl + far)}[side]
    elif place in BORDERS:          # (at most one level pixel between samples: the border's own texels are weighed)
        e = min(wide, 0.5 * rt)
        c = {'left': (-0.5 + jit(0.3), cym + jit(0.15 * spany)), 'right': (wl - 0.5 + jit(0.3), cym + jit(0.15 * spany)),
             'top': (cxm + jit(0.15 * spanx), -0.5 + jit(0.3)), 'bottom': (cxm + jit(0.15 * spanx), hl - 0.5 + jit(0.3))}[place]
    elif place in CORNERS:          # (samples 0.8 level pixels apart at most: one of them weighs the corner texel)
        e = min(wide, 0.4 * rt)
        c = ((0 if place[1] == 'l' else spanx) + jit(0.15), (0 if place[0] == 't' else spany) + jit(0.15))
    elif place == 'magnified':      # at most a quarter of a level pixel per output pixel
        e = rng.uniform(0.05, 0.24) * res / 2
        c = (cxm + jit(0.3 * spanx), cym + jit(0.3 * spany))
        theta = math.radians(jit(3.0))
    elif place == 'minified':       # the crop is twice the level: it covers the whole level plus a margin
        e = 1.0 * (max(hl, wl) + 1) + 2.0
        c = (cxm + jit(1.0), cym + jit(1.0))
        theta = math.radians(jit(3.0))
    elif place == 'inside':
        e = 0.22 * max(span, 0.5)
        c = (cxm + jit(0.1 * span), cym + jit(0.1 * span))
    else:                           # rotated, flipped, perspective: about the middle, may reach over the borders
        e = max(0.35 * span, 1.0)
        c = (cxm + jit(0.2 * spanx), cym + jit(0.2 * spany))
    if cls == 'rotated' or twist:
        theta = math.radians(rng.choice((-1, 1)) * rng.uniform(12.0, 35.0))
    if cls == 'flipped' or (twist and rng.random() < 0.5):
        flip = True
    if cls == 'perspective' or (twist and rng.random() < 0.5):
        persp = tuple(rng.choice((-1, 1)) * rng.uniform(0.5, 1.0) * 0.2 / rt for _ in range(2))
    s = 2 * e / rt                  # level pixels per sub-sample
    lin = s * _rot(theta) @ np.diag([-1.0 if flip else 1.0, 1.0])
    q0 = (rt - 1) / 2
    a = np.array([[lin[0, 0], lin[0, 1], 0], [lin[1, 0], lin[1, 1], 0], [persp[0], persp[1], 1]])
    t1 = np.array([[1, 0, -q0], [0, 1, -q0], [0, 0, 1.0]])
    t2 = np.array([[1, 0, c[0]], [0, 1, c[1]], [0, 0, 1.0]])
    m = t2 @ a @ t1                 # (U, V, 1) -> w * (position in level pixels, 1): position = c + lin q / w
    # the camera of the level: corner_aligned_scale_mat(2^-level) @ K with skew and non-square pixels; its principal
    # point lies 0.15 .. 0.3 focal lengths from the crop's centre, so that the distortion terms are all at work
    fl = 0.96 * full_side / 2 ** level * rng.uniform(0.95, 1.05)
    rho, phi = rng.uniform(0.15, 0.3), rng.uniform(0, 2 * math.pi)
    kl = np.array([[fl, jit(0.5) / 2 ** level, c[0] + rho * fl * math.cos(phi)],
                   [0, fl * rng.uniform(0.96, 1.04), c[1] + rho * fl * math.sin(phi)], [0, 0, 1.0]])
    hinv = np.linalg.inv(kl) @ m
    dist = _distortion(rng, dist_kind)
    wp = np.zeros(36, dtype=np.float32)
    wp[0:9], wp[9:18], wp[18:30] = hinv.reshape(9), kl.reshape(9), dist
    wp[30] = float(bool((wp[18:30] != 0).any()))
    wp[31], wp[32], wp[33], wp[34] = level, img, gexp, 1.0 / (s * aa)
    return dict(wp=wp, cls=cls, level=level, res=res, aa=aa, img=img, gexp=float(wp[33]), dist=dist_kind,
                rot=abs(theta) >= math.radians(12.0), flip=flip, persp=persp != (0.0, 0.0))


def positions(wp, res, aa, dtype=F64, hinv=None, swap_p=False):
    """Sample coordinates of the res*aa x res*aa sub-samples of a row, in pixels of its level: (ix, iy, oz, den)."""
    r = torch.as_tensor(np.asarray(wp, dtype=np.float32)).to(dtype)
    u = torch.arange(res * aa, dtype=dtype)
    V, U = torch.meshgrid(u, u, indexing='ij')
    h = r[0:9] if hinv is None else hinv.to(dtype).reshape(9)
    ox, oy, oz = h[0] * U + h[1] * V + h[2], h[3] * U + h[4] * V + h[5], h[6] * U + h[7] * V + h[8]
    nx, ny = ox / oz, oy / oz
    den = torch.ones_like(nx)
    if float(r[30]) != 0.0:
        d = r[18:30].clone()
        if swap_p:
            d[2], d[3] = r[21], r[20]
        r2 = nx * nx + ny * ny
        den = ((d[7] * r2 + d[6]) * r2 + d[5]) * r2 + 1
        a = (((d[4] * r2 + d[1]) * r2 + d[0]) * r2 + 1) / den
        b = 2 * (nx * d[3] + ny * d[2])
        cx, cy = (d[9] * r2 + d[3] + d[8]) * r2, (d[11] * r2 + d[2] + d[10]) * r2
        nx, ny = nx * (a + b) + cx, ny * (a + b) + cy
    k = r[9:18]
    return k[0] * nx + k[1] * ny + k[2], k[3] * nx + k[4] * ny + k[5], oz, den


def bilinear_zero(img, ix, iy):
    """Bilinear taps at direct pixel coordinates; a tap outside [0, W-1] x [0, H-1] contributes zero.  img [3,H,W]."""
    H, W = img.shape[1:]
    x0, y0 = torch.floor(ix), torch.floor(iy)
    tx, ty = ix - x0, iy - y0
    out = torch.zeros((3,) + ix.shape, dtype=img.dtype)
    for dy, wy in ((0, 1 - ty), (1, ty)):
        for dx, wx in ((0, 1 - tx), (1, tx)):
            xi, yi = x0 + dx, y0 + dy
            ok = (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)
            v = img[:, yi.clamp(0, H - 1).long(), xi.clamp(0, W - 1).long()]
            out = out + torch.where(ok, v * (wx * wy), torch.zeros_like(v))
    return out


def _pool_aa(x, res, aa):
    return x.reshape(3, res, aa, res, aa).mean(dim=(2, 4)) if aa > 1 else x


def yardstick(levels, row, dtype=F64):
    """The row's formula at `dtype` on the given pyramid levels (CPU tensors [N,3,H,W]) -> [3,res,res], linear light."""
    ix, iy, _, _ = positions(row['wp'], row['res'], row['aa'], dtype)
    img = levels[row['level']][row['img']].to(dtype)
    return _pool_aa(bilinear_zero(img, ix, iy), row['res'], row['aa'])


def oracle(levels, row, eval_dtype=None):
    """cpu_ref.warp_single_image on the row's matrices + the antialias avg_pool2d (multiperson_model.py:308-311); linear
    light.  eval_dtype=None: the reference's float32."""
    wp = torch.from_numpy(row['wp'])
    out = cpu_ref.warp_single_image(levels[row['level']][row['img']], wp[9:18].reshape(3, 3), wp[0:9].reshape(3, 3),
                                    wp[18:30], (row['res'] * row['aa'],) * 2, eval_dtype=eval_dtype)
    return F.avg_pool2d(out[None], row['aa'], row['aa'])[0] if row['aa'] > 1 else out


def has_degenerate_side(levels, row):
    return min(levels[row['level']].shape[2:]) < 2


def with_gamma(x, gexp):
    """crops **= gamma / 2.2 (multiperson_model.py:319) at x's own precision."""
    return x if gexp == 1.0 else x ** torch.tensor(gexp, dtype=x.dtype)


def reference32(levels, row):
    """The oracle's float32 evaluation of a row, gamma applied.  On a level with a side of 1 the oracle has no answer
    (module docstring): there, the direct formula in float32."""
    lin = yardstick(levels, row, torch.float32) if has_degenerate_side(levels, row) else oracle(levels, row)
    return with_gamma(lin, row['gexp'])


def direct32(levels, row):
    """A second, independent float32 evaluation: the direct-coordinate formula in float32, gamma applied."""
    return with_gamma(yardstick(levels, row, torch.float32), row['gexp'])


def _assert_domain_and_class(row, dims, n_images):
    """What the generator constructs, stated in fp64 on the packed (f32) row."""
    hl, wl = dims[row['level']]
    assert hl >= 1 and wl >= 1, 'a row names an empty level'
    assert 0 <= row['img'] < n_images and int(row['wp'][32]) == row['img']
    ix, iy, oz, den = positions(row['wp'], row['res'], row['aa'])
    assert float(oz.min()) > 0 and float(den.min()) > 0.5, (row['cls'], float(oz.min()), float(den.min()))
    x_lo, x_hi, y_lo, y_hi = float(ix.min()), float(ix.max()), float(iy.min()), float(iy.max())
    cls = 'br' if row['cls'] == 'last_br' else row['cls']
    outside = (ix <= -1) | (ix >= wl) | (iy <= -1) | (iy >= hl)
    if cls == 'inside':
        if min(hl, wl) >= 2:
            assert x_lo >= 0 and x_hi <= wl - 1 and y_lo >= 0 and y_hi <= hl - 1
        assert not bool(outside.any())
    elif cls == 'outside':
        assert bool(outside.all())
    elif cls == 'left':
        assert x_lo < -1 and x_hi > 0.5
    elif cls == 'right':
        assert x_hi > wl and x_lo < wl - 1.5
    elif cls == 'top':
        assert y_lo < -1 and y_hi > 0.5
    elif cls == 'bottom':
        assert y_hi > hl and y_lo < hl - 1.5
    elif cls in CORNERS:
        xc, yc = (0 if cls[1] == 'l' else wl - 1), (0 if cls[0] == 't' else hl - 1)
        assert bool((((ix - xc).abs() < 1) & ((iy - yc).abs() < 1)).any()), 'no sample weighs the corner texel'
        assert bool(outside.any())
    elif cls == 'magnified':
        step = math.hypot(float(ix[0, -1] - ix[0, 0]), float(iy[0, -1] - iy[0, 0])) / (ix.shape[1] - 1) * row['aa']
        assert step <= 0.25, step
    elif cls == 'minified':
        assert x_lo <= -1 and x_hi >= wl and y_lo <= -1 and y_hi >= hl
    if row['flip']:
        ax, ay = float(ix[0, 1] - ix[0, 0]), float(iy[0, 1] - iy[0, 0])
        bx, by = float(ix[1, 0] - ix[0, 0]), float(iy[1, 0] - iy[0, 0])
        assert ax * by - ay * bx < 0
    if row['persp']:
        assert row['wp'][6] != 0 and row['wp'][7] != 0


def _build_set(index, n, h, w):
    rng = random.Random(SEED + index)
    dims = level_dims(h, w)
    live = [l for l in range(3) if dims[l][0] >= 1 and dims[l][1] >= 1]
    sizes = [rng.choice((9, 10, 11)), rng.choice((5, 6, 7)), rng.choice((3, 4, 5))]   # never a multiple of 8, nor their sum
    groups = [(RES[(3 * index + g) % len(RES)], ((1, 2)[index % 2], (4, 1, 4)[index % 3], (2, 4, 1)[index % 3])[g])
              for g in range(3)]
    n_rows = sum(sizes)
    classes = list(CLASSES) + [rng.choice(BORDERS + CORNERS + ('rotated',)) for _ in range(n_rows - len(CLASSES))]
    twists = [False] * len(CLASSES) + [True] * (n_rows - len(CLASSES))
    order = list(range(n_rows))
    rng.shuffle(order)
    levels = [live[i % len(live)] for i in range(n_rows)]
    rng.shuffle(levels)
    kinds = [('none', 'd5', 'd12')[i % 3] for i in range(n_rows)]
    rng.shuffle(kinds)
    group_of = [g for g, size in enumerate(sizes) for _ in range(size)]
    rows = []
    for pos, j in enumerate(order):
        res, aa = groups[group_of[pos]]
        cls = classes[j]
        img = n - 1 if cls == 'last_br' else rng.randrange(n)
        gexp = 1.0 if pos % 2 == 0 else tta_exponent(rng.randrange(4))
        row = _make_row(rng, dims, max(h, w), levels[pos], cls, res, aa, img, gexp, kinds[pos], twists[j])
        row['group'], row['kernel'] = group_of[pos], kernel_pool(h, w, aa)
        _assert_domain_and_class(row, dims, n)
        rows.append(row)
    return dict(name=f'{n}x{h}x{w}', n=n, h=h, w=w, dims=dims, seed=SEED + index, rows=rows, groups=groups)


_SETS = None


def frame_sets():
    global _SETS
    if _SETS is None:
        _SETS = [_build_set(i, *shape) for i, shape in enumerate(FRAME_SETS)]
    return _SETS


def frames_of(fs):
    """uint8 [N,3,H,W]; even frames are noise: a wrong texel is loud."""
    return cases.synth_images(fs['n'], fs['h'], fs['w'], fs['seed'])


def cpu_pyramid(level0):
    """F.avg_pool2d 2x2 twice (warping.py:10-13); a level without rows or columns -- avg_pool2d refuses to make one -- is
    an empty tensor of its shape."""
    levels = [level0]
    for _ in range(2):
        n, c, h, w = levels[-1].shape
        levels.append(F.avg_pool2d(levels[-1], 2, 2) if h >= 2 and w >= 2 else levels[-1].new_zeros(n, c, h // 2, w // 2))
    return levels


def group_rows(fs, g):
    """(indices, [n,36] float32 tensor, res, aa) of launch g of a frame set: the rows that share (res, aa)."""
    idx = [i for i, r in enumerate(fs['rows']) if r['group'] == g]
    res, aa = fs['groups'][g]
    return idx, torch.from_numpy(np.stack([fs['rows'][i]['wp'] for i in idx])), res, aa


# ---- the checker

def _linear(x, gexp):
    x = x.double()
    return x if gexp == 1.0 else x.clamp_min(0) ** (1.0 / gexp)   # as test_geometry_and_get_crops_vs_oracle undoes it


class Report:
    def __init__(self):
        self.lines, self.failures, self.bad_rows, self.pools = [], [], [], {}

    @property
    def ok(self):
        return not self.failures


def check(name, rows, ours, truth64, ref32):
    """ours / ref32: per row [3,res,res] with the row's gamma applied; truth64: per row, linear light.  Pools: per kernel.
    max and mean of |ours - truth64| <= 4 x those of |ref32 - truth64| + 8 * 2^-24; a row entirely outside the frame is
    exactly zero.  -> Report (lines: the [parity] figures; bad_rows: rows beyond their pool's max bound or not zero)."""
    rep = Report()
    errs = {}
    for i, row in enumerate(rows):
        assert ours[i].shape == truth64[i].shape == ref32[i].shape == (3, row['res'], row['res'])
        assert bool(torch.isfinite(ref32[i]).all()), 'the reference has no answer for this row: it is outside the domain'
        eo = (_linear(ours[i], row['gexp']) - truth64[i]).abs()
        er = (_linear(ref32[i], row['gexp']) - truth64[i]).abs()
        eo = torch.where(torch.isfinite(eo), eo, torch.full_like(eo, float('inf')))
        errs.setdefault(row['kernel'], []).append((i, eo, er))
        if row['cls'] == 'outside' and not bool((ours[i] == 0).all()):
            rep.failures.append(f'{name} row {i}: entirely outside the frame but not exactly zero')
            rep.bad_rows.append(i)
    for pool, items in sorted(errs.items()):
        eo_all, er_all = torch.cat([e.flatten() for _, e, _ in items]), torch.cat([e.flatten() for _, _, e in items])
        o_max, o_mean, r_max, r_mean = (float(v) for v in (eo_all.max(), eo_all.mean(), er_all.max(), er_all.mean()))
        b_max, b_mean = MARGIN * r_max + ABS_FLOOR, MARGIN * r_mean + ABS_FLOOR
        rep.pools[pool] = dict(ours_max=o_max, ours_mean=o_mean, ref_max=r_max, ref_mean=r_mean)
        rep.lines.append(
            f'[parity] sampler fuzz {name} {pool} ({len(items)} rows): ours / reference max {o_max / max(r_max, 1e-300):.2f} '
            f'mean {o_mean / max(r_mean, 1e-300):.2f}; reference floor max {r_max:.2e} mean {r_mean:.2e}; ours max '
            f'{o_max:.2e} mean {o_mean:.2e}')
        if not o_max <= b_max:
            rep.failures.append(f'{name} {pool}: max {o_max:.3e} > {b_max:.3e} (4 x {r_max:.3e} + 8 * 2^-24)')
        if not o_mean <= b_mean:
            rep.failures.append(f'{name} {pool}: mean {o_mean:.3e} > {b_mean:.3e} (4 x {r_mean:.3e} + 8 * 2^-24)')
        rep.bad_rows += [i for i, eo, _ in items if not float(eo.max()) <= b_max and i not in rep.bad_rows]
    return rep


# ---- wrong references

WRONG = ('last_column_zeroed', 'last_row_zeroed', 'first_column_zeroed', 'border_padding', 'align_corners_false',
         'neighbouring_level', 'p1_p2_swapped', 'next_image', 'aa_without_shift', 'neighbours_gamma')


def wrong_applies(variant, fs, i):
    """Whether the wrong variant is a DIFFERENT function on row i of the frame set (not: whether it differs enough)."""
    row = fs['rows'][i]
    hl, wl = fs['dims'][row['level']]
    if variant == 'align_corners_false':
        return hl >= 2 and wl >= 2
    if variant == 'neighbouring_level':
        return True   # every frame set has at least levels 0 and 1
    if variant == 'p1_p2_swapped':
        return row['wp'][30] != 0 and row['wp'][20] != row['wp'][21]
    if variant == 'next_image':
        return fs['n'] >= 2
    if variant == 'aa_without_shift':
        return row['aa'] >= 2
    if variant == 'neighbours_gamma':
        return fs['rows'][(i + 1) % len(fs['rows'])]['gexp'] != row['gexp']
    return True


def wrong(variant, fs, levels, i):
    """Row i of a frame set evaluated in fp64 with one thing wrong, gamma applied (what a subtly wrong kernel returns)."""
    row = dict(fs['rows'][i])
    res, aa, gexp = row['res'], row['aa'], row['gexp']
    lv = row['level']
    img = levels[lv][row['img']].double().clone()
    hl, wl = img.shape[1:]
    kw = {}
    if variant == 'last_column_zeroed':
        img[:, :, -1] = 0
    elif variant == 'last_row_zeroed':
        img[:, -1, :] = 0
    elif variant == 'first_column_zeroed':
        img[:, :, 0] = 0
    elif variant == 'neighbouring_level':
        other = lv + 1 if lv + 1 < 3 and levels[lv + 1].shape[2] * levels[lv + 1].shape[3] > 0 else lv - 1
        img = levels[other][row['img']].double()
    elif variant == 'next_image':
        img = levels[lv][(row['img'] + 1) % fs['n']].double()
    elif variant == 'p1_p2_swapped':
        kw['swap_p'] = True
    elif variant == 'aa_without_shift':
        # Hinv = H @ corner_aligned_scale_mat(1 / aa) (warping.py:128-133); without its shift: H @ diag(1/aa, 1/aa, 1)
        f = 1.0 / aa
        s_mat = torch.tensor([[f, 0, (f - 1) / 2], [0, f, (f - 1) / 2], [0, 0, 1]], dtype=F64)
        h = torch.from_numpy(row['wp'][0:9]).double().reshape(3, 3)
        kw['hinv'] = h @ torch.linalg.inv(s_mat) @ torch.diag(torch.tensor([f, f, 1.0], dtype=F64))
    elif variant == 'neighbours_gamma':
        gexp = fs['rows'][(i + 1) % len(fs['rows'])]['gexp']
    ix, iy, _, _ = positions(row['wp'], res, aa, **kw)
    if variant == 'border_padding':
        ix, iy = ix.clamp(0, wl - 1), iy.clamp(0, hl - 1)
    elif variant == 'align_corners_false':   # grid_sample's un-normalisation ((x + 1) * size - 1) / 2 of x = 2 ix / (size - 1) - 1
        ix, iy = ix * wl / (wl - 1) - 0.5, iy * hl / (hl - 1) - 0.5
    return with_gamma(_pool_aa(bilinear_zero(img, ix, iy), res, aa), gexp)


# ---- crop_geometry

GEOMETRY_FRAME = (2, 97, 131)
GEOMETRY_SEED = 70707
N_GEOMETRY = 24
BOX_KINDS = ('inside', 'partly', 'far', 'thin', 'larger')
UP_KINDS = ('default', 'tilted', 'parallel')
GEOMETRY_RES = (7, 18, 33, 40, 64, 100, 256, 384)
GEOMETRY_AAS = (1, 2, 4, 8)
THRESHOLDS = [(k, u) for k in (0, 1, 2) for u in (-2, -1, 0, 1, 2)]   # hand-made scales f32(2^-k / box_scale) + u ulp


def _geometry_camera(rng, h, w, exact):
    if exact:   # power-of-two focal lengths, no skew: inv(K) @ (principal point) is EXACTLY (0, 0, 1) in any arithmetic
        return np.array([[128.0, 0, 64.5], [0, 64.0, 48.25], [0, 0, 1]])
    f = 0.96 * max(h, w) * rng.uniform(0.9, 1.1)
    return np.array([[f, rng.uniform(-0.8, 0.8), w / 2 + rng.uniform(-4, 4)],
                     [0, f * rng.uniform(0.9, 1.1), h / 2 + rng.uniform(-4, 4)], [0, 0, 1.0]])


def _geometry_box(rng, kind, h, w):
    j = lambda a: rng.uniform(-a, a)
    if kind == 'inside':
        return [30 + j(5), 20 + j(5), 40 + j(5), 55 + j(5)]
    if kind == 'partly':
        return [-15 + j(5), 50 + j(5), 60 + j(5), 70 + j(5)]
    if kind == 'far':
        return [w * 1.6 + j(5), -h * 0.9 + j(5), 50 + j(5), 80 + j(5)]
    if kind == 'thin':
        return [60 + j(5), 15 + j(5), 1.0, 60 + j(5)]
    return [-40 + j(5), -30 + j(5), w + 90 + j(5), h + 70 + j(5)]


def _build_geometry_cases():
    rng = random.Random(GEOMETRY_SEED)
    n, h, w = GEOMETRY_FRAME
    out = []
    thresholds = list(THRESHOLDS) * 4
    for i in range(N_GEOMETRY):
        up_kind = UP_KINDS[2] if i % 6 == 5 else UP_KINDS[i % 2]
        kind = 'inside' if up_kind == 'parallel' else BOX_KINDS[i % len(BOX_KINDS)]
        dist_kind = 'none' if up_kind == 'parallel' else ('none', 'd5', 'd12')[(i // 2) % 3]
        K = _geometry_camera(rng, h, w, up_kind == 'parallel')
        box = _geometry_box(rng, kind, h, w)
        if up_kind == 'parallel':   # centred on the principal point, in numbers that halve exactly
            bw, bh = 32.0 + 2 * (i % 5), 48.0 + 2 * (i % 3)
            box = [K[0, 2] - bw / 2, K[1, 2] - bh / 2, bw, bh]
        # (far / larger boxes: the canonical signs, whose radial factor stays above 0.75 at any radius -- with drawn
        #  signs the five fixed-point iterations of undistort_points can run into its zero)
        dist = _distortion(rng, dist_kind, signs_drawn=kind not in ('far', 'larger'))
        up = {'default': (0.0, -1.0, 0.0), 'tilted': (0.2, -0.95, 0.1),
              'parallel': (0.0, 0.0, 1.0 if i % 12 == 5 else -1.0)}[up_kind]
        cols = 4 + (i // 3) % 2
        n_tta, n_hand = 1 + i % 4, (0, 1, 2, 3)[(i // 4) % 4] if i % 4 != 3 else 2
        # the companion: a plain box with its own camera, before or behind the case's box (per-box indexing)
        K2 = _geometry_camera(rng, h, w, False)
        box2 = _geometry_box(rng, 'inside', h, w)
        first = i % 2 == 0
        boxes = np.zeros((2, cols), dtype=np.float32)
        boxes[:, 4:] = 1.0   # a confidence column, never read
        boxes[0 if first else 1, :4], boxes[1 if first else 0, :4] = box, box2
        pick = lambda a, b: np.stack([a, b] if first else [b, a]).astype(np.float32)
        res = GEOMETRY_RES[i % len(GEOMETRY_RES)]
        aa = GEOMETRY_AAS[(i // 2) % len(GEOMETRY_AAS)]
        warp = kind in ('inside', 'partly', 'thin') and res <= 40 and aa <= 4
        out.append(dict(
            index=i, kind=kind, up_kind=up_kind, dist=dist_kind, cols=cols, res=res, aa=aa, slot=0 if first else 1,
            boxes=boxes, K=pick(K, K2), dist12=pick(dist, np.zeros(12)), up=pick(np.array(up), np.array([0.0, -1.0, 0.0])),
            ids=np.array([i % n, (i + 1) % n], dtype=np.int32), n_tta=n_tta,
            hand=[thresholds.pop(0) for _ in range(n_hand)], warp=warp))
    return out


_GEOMETRY = None


def geometry_cases():
    global _GEOMETRY
    if _GEOMETRY is None:
        _GEOMETRY = _build_geometry_cases()
    return _GEOMETRY


def geometry_inputs(case):
    """The arguments of kernels.crop_geometry but the augmentations, as CPU tensors."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return dict(boxes=t(case['boxes']), K=t(case['K']), dist12=t(case['dist12']), up=t(case['up']), ids=t(case['ids']))


def ulp_steps(x32, steps):
    x = np.float32(x32)
    for _ in range(abs(steps)):
        x = np.nextafter(x, np.float32(np.inf if steps > 0 else 0), dtype=np.float32)
    return x


def geometry_augmentations(case, box_scale):
    """rotflipmat [A,3,3], scales [A], gammas [A]: n_tta rows of cpu_ref.tta_params, then the hand-made scales
    f32(2^-k / box_scale) + u ulp (rotation / flip and gamma of the TTA rows in turn).  box_scale: the f32 the kernel
    wrote into [34] of the case's row in a first call with scale 1; None for that first call (scales of 1)."""
    tta = cpu_ref.tta_params(case['n_tta'])
    rf, sc, ga = [tta['rotflipmat']], [tta['scales']], [tta['gammas']]
    for j, (k, u) in enumerate(case['hand']):
        rf.append(tta['rotflipmat'][j % case['n_tta']][None])
        ga.append(tta['gammas'][j % case['n_tta']][None])
        s = 1.0 if box_scale is None else float(ulp_steps(np.float32(2.0 ** -k / float(box_scale)), u))
        sc.append(torch.tensor([s], dtype=torch.float32))
    scales = torch.cat(sc).float()
    if box_scale is None:
        scales = torch.ones_like(scales)
    return dict(rotflipmat=torch.cat(rf).float(), scales=scales, gammas=torch.cat(ga).float())


def exact_level(scale32, aa):
    """clip(floor(-log2(f32(scale * aa))), 0, 2) evaluated exactly: aa is a power of two, so the product is exact in f32
    (no overflow at these sizes), and floor(-log2 x) is 0 for x > 1/2, 1 for 1/4 < x <= 1/2, 2 for x <= 1/4."""
    x = float(np.float32(scale32) * np.float32(aa))
    return 0 if x > 0.5 else (1 if x > 0.25 else 2)


def geometry_oracle64(case, aug, scales32=None):
    """The oracle's formulas (cpu_ref.get_new_rotation_and_scale, get_crops) run on float64 tensors.  -> dict:
    crop_scale [A,n] (fp64, from the inputs alone) and, recomputed from `scales32` [A,n] (the f32 crop scale of the
    rows under test; default: crop_scale rounded to f32), new_k, rot, hinv, k_level [A,n,3,3], level [A,n]."""
    inp = geometry_inputs(case)
    K, d12, up = inp['K'].double(), inp['dist12'].double(), inp['up'].double()
    with torch.inference_mode():
        r_noaug, box_scales = cpu_ref.get_new_rotation_and_scale(K, d12, up, inp['boxes'][:, :4].double(), case['res'])
    crop_scale = aug['scales'].double()[:, None] * box_scales[None, :]
    s32 = crop_scale.float() if scales32 is None else scales32.float().reshape(crop_scale.shape)
    s = s32.double()
    A, n = s.shape
    res, aa = case['res'], case['aa']
    new_k = torch.zeros(A, n, 3, 3, dtype=F64)
    new_k[:, :, :2, :2] = K[None, :, :2, :2] * s[:, :, None, None]
    new_k[:, :, :2, 2] = res / 2
    new_k[:, :, 2, 2] = 1
    rot = aug['rotflipmat'].double()[:, None] @ r_noaug[None]
    hinv = torch.linalg.inv(new_k @ rot)
    if aa > 1:
        f = 1.0 / aa
        hinv = hinv @ torch.tensor([[f, 0, (f - 1) / 2], [0, f, (f - 1) / 2], [0, 0, 1]], dtype=F64)
    level = torch.tensor([[exact_level(float(s32[a, b]), aa) for b in range(n)] for a in range(A)])
    fl = 1.0 / 2.0 ** level.double()
    scale_mats = torch.zeros(A, n, 3, 3, dtype=F64)
    scale_mats[..., 0, 0] = scale_mats[..., 1, 1] = fl
    scale_mats[..., 0, 2] = scale_mats[..., 1, 2] = (fl - 1) / 2
    scale_mats[..., 2, 2] = 1
    return dict(crop_scale=crop_scale, box_scales=box_scales, r_noaug=r_noaug, new_k=new_k, rot=rot, hinv=hinv,
                k_level=scale_mats @ K[None], level=level, gexp=aug['gammas'].numpy() / np.float32(2.2))


def matrix_bound(m64):
    """Bound on |f32 entry of the kernel - fp64 entry| for new_k, rot, Hinv and K_level [..,3,3].  The kernel evaluates
    the same formulas in fp64 and rounds ONCE: half an f32 ulp of the entry, plus the distance between two fp64
    evaluations (orders below an f32 ulp of the matrix's largest entry) -- 1 ulp of the entry leaves room for that and
    for a tie.  An entry that is a difference of larger terms (a rotation's small components, the translation column
    of the inverse) carries the fp64 error of those terms, not of itself: its bound is 2^-24 of the matrix's largest
    entry (half an f32 ulp of that entry at most) where that is the larger of the two."""
    return torch.maximum(cases.f32_ulp_at(m64), 2.0 ** -24 * m64.abs().amax(dim=(-2, -1), keepdim=True).expand_as(m64))


def scale_bound(s64):
    """The crop scale is rounded twice -- box_scale to f32, then its f64 product with the augmentation's scale to f32 --
    half an ulp each (the first one relative, carried through the product): 2 ulp covers both and the binade edge."""
    return 2 * cases.f32_ulp_at(s64)

"""Seeded fuzz of the fused head (mtr_head_fused_ws: csrc/head_rt.hip, head_fused.hip, head_areg.hip, head_res.hip,
head_pp.hip, head16.h) and of the stand-alone decode (mtr_softargmax_decode_opts: csrc/decode.hip) over the domain
their entry points accept: a helper of tests/test_head_fuzz_host.py (CPU) and tests/test_gpu_head_fuzz.py (GPU), no
test module itself.

Four families (FAMILIES), N_CASES cases each from random.Random(a fixed seed) -- Python's generator, so the draws do
not move with the torch version:

    head32    f32 features, both layouts          H*W % 4 == 0; D <= 80; NHWC: C % 4 == 0
    head16    f16 / bf16, the joint-group kernels C % 8 == 0; 1 + D <= 64; H*W <= 256; H*W % 4 == 0
    head16rt  f16 / bf16 on the row-tile core     C % 64 == 0; D <= 80; 1 + D > 64 or H*W > 256
    decode    f32 / f16 / bf16 logits, both layouts, nhwc_staging 0 .. 3: any H, W, J, D >= 1

A case is a dict: the shape, the dtype, the layout, one head config and one input kind.  Every case lies inside its
entry point's domain BY CONSTRUCTION: a value is drawn from the values the family's rules allow (C of an NHWC head32
case from the multiples of 4, D of a head16 case from the D <= 63, a head16rt case either a deep D with any map or a
map of more than 256 positions with any D) -- nothing is drawn and rejected.  The shapes are the smallest at which a
mechanism of the kernels changes behaviour (the comments at B_VALUES .. MAPS), never the workload's own.

  * cases(family); inputs(case): CPU tensors -- the features AS CONSUMED (rounded to the case's dtype), f32 weights
    and bias, or the logits;
  * on_device(case, inputs, nhwc=, crops=): the same on the GPU (in either layout, or a slice of the batch), the
    features / logits carved from NaN-filled buffers;
  * reference(case, inputs) -> (coords2d, coords3d_rel) in fp64: cpu_ref.heads_from_logits(eval_dtype=float64) on
    the fp64 product of the operands as the kernel consumes them (f32 features and weights; 16-bit features with
    cases.head_weights_as_consumed).  No decode arithmetic is restated here: the softmax and the axis coordinates of
    the bound are cpu_ref.joint_softmax and cpu_ref.ref_linspace (an axis of one element decodes to 0.5);
  * bound(case, inputs): a derived bound on EVERY output element, below;
  * wrong(kind, case, inputs): subtly wrong fp64 answers from the same reference function (WRONG, wrong_applies);
  * run(kernels, case, dev, out=, workspace=, **options): the launch through metrabs_amd.kernels;
  * variants(kernels, case): the option dicts whose kernels.head_plan reports a kernel or tiling not yet in the list.

THE BOUND.  |got - fp64| <= bound per element, u = 2^-24:

 1. Logits (fused families; e_L = 0 for decode, whose logits are the input).  For ANY summation order of the f32
    sums -- chains of 32 channels carried into f64, MFMA accumulators, two K groups --
        e_L = (C + 2) u (|W| |x| + |b|) + u |L|
    (the form of tests/test_gpu_backbone16.py: C products and C - 1 additions of relative error u each, the bias and
    the final rounding; the products of two 16-bit operands are exact in f32).
 2. Through the softmax, exactly (not to first order).  With p the fp64 softmax of a unit, E = sum p c and
    eps = max e_L over the unit:  |E' - E| <= exp(eps) * sum_i p_i |c_i - E| (exp(e_L,i) - 1).
    (E' - E = sum p_i g_i (c_i - E) / sum p_i g_i with g_i = exp(delta_i) in [exp(-eps), exp(eps)]; subtract
    sum p_i (c_i - E) = 0 from the numerator: |sum p_i (g_i - 1)(c_i - E)| <= sum p_i |c_i - E| (exp(e_L,i) - 1); the
    denominator is at least exp(-eps).)
 3. The kernel's own evaluation.  Every term of the three sums is non-negative, so any order of n terms costs at most
    about n u relative (the sums are f64 in every kernel: far less; n u is what the f32 oracle needs), and the
    exponential carries a relative error eta_i = (EXP_A + EXP_B |L_i - m|) u:
        sum p_i c_i eta_i + E sum p_i eta_i + (2 (n + 4) + 4) u E.
    EXP_A = 8, EXP_B = 2, read off exp_shifted (csrc/common.h): e = v_exp_f32(fma(x, log2e_f, -m log2e_f)).
      - the fma rounds its result t = (x - m) log2 e once: |dt| <= u |t|, a factor exp(ln 2 dt) on e: u |x - m|;
      - log2e_f is log2 e rounded to f32 (relative error 1.2e-8 = 0.2 u): in the fma its error multiplies x - m, for
        the product m log2e_f uses the same constant: 0.2 u |x - m|.  Together < EXP_B |x - m| u;
      - v_exp_f32 is accurate to 1 ulp = 2 u relative, and the result is widened to f64 exactly; a result below
        2^-126 is flushed to zero: at most n 2^-126 on a sum of at least 1/2, which the floor (5.) covers.
        EXP_A = 8 leaves 6 u for the f64 polynomial exp_neg64 of the merges (1e-16 each, at most a few per block),
        the reciprocal of the sum and the rounding of the coordinate to f32;
      - -m log2e_f is rounded ONCE per row tile or column block: its error, at most u |m_block|, is a common factor
        of that block's terms only, and terms of different blocks of one unit carry different factors.  It does not
        cancel between blocks, so u * max|L| of the unit is ADDED to eta.
    The f64 paths (MTR_RT_EXP32 = 0, ACC64 of head16.h) evaluate exp_neg64 on the f64 difference: inside the same eta.
 4. The epilogue (heatmap_to_px, heatmap_to_mm_xy, heatmap_to_mm_z of csrc/common.h): the three terms scaled by
    last_center (times box_size_mm / proc_side for mm) or by box_size_mm for z; one rounding for each __fmul_rn,
    __fadd_rn, __fdiv_rn -- at most five, every intermediate non-negative and no larger than the result: 5 u |value|.
 5. An absolute floor of 2^-100 times the scale (a coordinate whose fp64 value is 1e-60 is exactly 0 in f32).
"""
import random

import torch

from oracle import cases as oracle_cases
from oracle import cpu_ref

SEED = 52525
N_CASES = 24
FAMILIES = ('head32', 'head16', 'head16rt', 'decode')
F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
GUARD = 256           # elements on either side of a guarded tensor: its base stays 16-byte aligned
SENTINEL = -32768.0   # exact in f32, and far outside every result
U = 2.0 ** -24
EXP_A, EXP_B = 8.0, 2.0
FLOOR = 2.0 ** -100

# the 8-crop chunk, and B % 4 in {1, 2, 3} for the packed last blocks
B_VALUES = (1, 2, 3, 5, 7, 8, 9)
# seven joints fill a 64-row group at D = 8; 8 and 17 overflow the atoms of D = 8 / D = 16 with 2D rows; odd counts
# leave a ragged last atom
J_VALUES = (1, 2, 3, 5, 7, 8, 15, 17)
J_SMALL = (1, 2, 3, 5)      # with D >= 31: a case stays a few hundred output rows
# one-tile atoms with 16, 8, 5, 3, 2 and 1 units, 0 and several free rows; atoms of 2 .. 5 tiles; 3, 2 and 1 joints
# per 64-row group
D_VALUES = (1, 2, 3, 5, 8, 15, 16, 17, 20, 31, 33, 48, 63)
D_DEEP = (64, 65, 72, 80)
# odd and even stage counts, C % 32 and C % 64 of the loader wave and of the two K groups
C_HEAD32 = (1, 4, 31, 32, 33, 63, 64, 65, 96, 100, 128, 132)
# fewer stages than the prefetch depth, whole and ragged 64-channel stages
C_HEAD16 = (8, 24, 56, 64, 72, 128, 192, 200)
C_HEAD16RT = (64, 128, 192)
C_RESIDENT = 1280           # the resident-weights kernel takes nothing else
# H*W -> (H, W): less than one, exactly one and several 64-position column blocks; last blocks of 16 and of 32
# positions (the packed ones); every count of 32-position column tiles 1 .. 8 (192: six, which the other sizes miss);
# two rectangles for every square
MAPS = {4: ((1, 4), (4, 1), (2, 2)), 16: ((2, 8), (8, 2), (4, 4)), 32: ((4, 8), (8, 4), (2, 16)),
        36: ((4, 9), (3, 12), (6, 6)), 60: ((6, 10), (5, 12), (10, 6)), 64: ((4, 16), (16, 4), (8, 8)),
        68: ((4, 17), (17, 4), (2, 34)), 80: ((8, 10), (10, 8), (5, 16)), 96: ((8, 12), (12, 8), (6, 16)),
        100: ((5, 20), (20, 5), (10, 10)), 128: ((8, 16), (16, 8), (4, 32)), 132: ((11, 12), (12, 11), (6, 22)),
        144: ((9, 16), (16, 9), (12, 12)), 160: ((10, 16), (16, 10), (8, 20)), 192: ((12, 16), (16, 12), (8, 24)),
        196: ((7, 28), (28, 7), (14, 14)), 224: ((14, 16), (16, 14), (8, 28)), 256: ((8, 32), (32, 8), (16, 16)),
        # five and more column blocks: a workgroup tile of up to four wraps
        260: ((13, 20), (20, 13), (10, 26)), 288: ((16, 18), (18, 16), (12, 24)), 400: ((16, 25), (25, 16), (20, 20))}
HW_SMALL = tuple(hw for hw in MAPS if hw <= 256)
HW_LARGE = (260, 288, 400)
HW_RESIDENT = (96, 128, 144, 160)   # 3 .. 5 column tiles, whole 16-byte chunks per NCHW channel row
# decode: odd maps, widths that are a multiple of neither 4 nor 8, single rows and columns
MAPS_DECODE = ((5, 5), (1, 7), (3, 9), (7, 1), (1, 1), (6, 7), (9, 10), (5, 13), (2, 3), (11, 6), (13, 21), (20, 19))
STRIDES = (4, 8, 16, 32)
PROC_KINDS = ('exact', 'minus3', 'minus_half')
FLAGS = ((True, False), (False, False), (True, True), (False, True))    # (centered_stride, legacy_centered_stride_bug)
BOXES = (2200.0, 1000.0, 3131.5)
KINDS = ('flat', 'gain', 'spike', 'two_peaks', 'level')
SPIKES = (20.0, 60.0, 150.0)
PEAKS = (160.0, 60.0)       # two logits of one unit, 100 apart


# ---- draws

def _balanced(rng, values, n=N_CASES):
    """n values, every one of `values` as often as the others (to within one), in a shuffled order."""
    out = [values[i % len(values)] for i in range(n)]
    rng.shuffle(out)
    return out


def _head_config(case, stride, proc_kind, flags, box):
    base = max(case['H'], case['W']) * stride
    proc = {'exact': base, 'minus3': base - 3, 'minus_half': base - stride // 2}[proc_kind]
    case.update(stride=stride, proc_kind=proc_kind, proc_side=proc, centered=flags[0], legacy=flags[1], box=box)


def _finish(family, rng, rows):
    """The head config and the input kind of every case: each balanced over the family's 24 cases on its own."""
    strides, procs = _balanced(rng, STRIDES), _balanced(rng, PROC_KINDS)
    flags, boxes = _balanced(rng, FLAGS), _balanced(rng, BOXES)
    kinds = _balanced(rng, KINDS)
    gains = {'flat': _balanced(rng, (1.0, 3.0)), 'gain': _balanced(rng, (10.0, 30.0))}
    count = {k: 0 for k in KINDS}
    for i, c in enumerate(rows):
        c.update(family=family, index=i)
        _head_config(c, strides[i], procs[i], flags[i], boxes[i])
        if i == 0:    # CONFIG_S_256's combination
            c.update(stride=32, proc_side=256, centered=False, legacy=True, box=2200.0)
        if i == 1:    # CONFIG_L_384's
            c.update(stride=32, proc_side=384, centered=True, legacy=False, box=2200.0)
        kind = kinds[i]
        n = count[kind]
        count[kind] += 1
        c.update(kind=kind, gain=gains.get(kind, gains['flat'])[i], seed=SEED + 1000 * FAMILIES.index(family) + i)
        # the input scale where a wrong answer would otherwise lie within 10 bounds of the right one -- rules on the
        # case: the bound's allowance for an f32 sum of n terms grows with n while a flat unit's sensitivity to its
        # logits falls as 1 / sqrt(n): units of 8192 terms and more take the larger flat gain; and a gain of 30 on a
        # map of several hundred positions leaves one position of a unit with any weight (its last column block
        # weighs nothing): such maps take 10
        if kind != 'gain' and c['D'] * c['H'] * c['W'] >= 8192:
            c.update(gain=3.0)
        if kind == 'gain' and c['H'] * c['W'] > 256:
            c.update(gain=10.0)
        if kind == 'spike':
            c.update(amp=SPIKES[n % len(SPIKES)], rotation=n % 4)
        if kind == 'two_peaks':
            c.update(larger_first=n % 2 == 0)     # the larger peak in the earlier block, then in the later one
        if kind == 'level':
            c.update(level_3d=n % 2 == 0)
    return rows


def _map(rng, hw):
    return rng.choice(MAPS[hw])


def _joints(rng, D, pool):
    return pool if D < 31 else rng.choice(J_SMALL)


def _cases_head32(rng):
    Bs, Js = _balanced(rng, B_VALUES), _balanced(rng, J_VALUES)
    Ds, hws = _balanced(rng, D_VALUES + D_DEEP), _balanced(rng, tuple(MAPS))
    nhwc = _balanced(rng, (False, True))
    c_any, c_mult4 = _balanced(rng, C_HEAD32), _balanced(rng, tuple(c for c in C_HEAD32 if c % 4 == 0))
    rows = []
    for i in range(N_CASES):
        H, W = _map(rng, hws[i])
        rows.append(dict(B=Bs[i], C=(c_mult4 if nhwc[i] else c_any)[i], J=_joints(rng, Ds[i], Js[i]), D=Ds[i], H=H, W=W,
                         dtype=F32, nhwc=nhwc[i]))
    return rows


def _cases_head16(rng):
    Bs, Js = _balanced(rng, B_VALUES), _balanced(rng, J_VALUES)
    Ds, hws = _balanced(rng, D_VALUES), _balanced(rng, HW_SMALL)
    nhwc, dts, Cs = _balanced(rng, (False, True)), _balanced(rng, (F16, BF16)), _balanced(rng, C_HEAD16)
    rows = []
    for i in range(N_CASES):
        H, W = _map(rng, hws[i])
        rows.append(dict(B=Bs[i], C=Cs[i], J=_joints(rng, Ds[i], Js[i]), D=Ds[i], H=H, W=W, dtype=dts[i], nhwc=nhwc[i]))
    H, W = _map(rng, rng.choice(HW_RESIDENT))
    rows[2].update(B=2, C=C_RESIDENT, J=rng.choice((2, 3)), D=8, H=H, W=W)
    return rows


def _cases_head16rt(rng):
    Bs, Js = _balanced(rng, B_VALUES), _balanced(rng, J_VALUES)
    nhwc, dts, Cs = _balanced(rng, (False, True)), _balanced(rng, (F16, BF16)), _balanced(rng, C_HEAD16RT)
    deep = _balanced(rng, (True, False))        # which of the two rules puts the case on the row-tile core
    d_deep, d_any = _balanced(rng, D_DEEP), _balanced(rng, D_VALUES + D_DEEP)
    hw_any, hw_large = _balanced(rng, tuple(MAPS)), _balanced(rng, HW_LARGE)
    rows = []
    for i in range(N_CASES):
        D = d_deep[i] if deep[i] else d_any[i]
        H, W = _map(rng, hw_any[i] if deep[i] else hw_large[i])
        rows.append(dict(B=Bs[i], C=Cs[i], J=_joints(rng, D, Js[i]), D=D, H=H, W=W, dtype=dts[i], nhwc=nhwc[i]))
    return rows


def _cases_decode(rng):
    Bs, Js = _balanced(rng, B_VALUES), _balanced(rng, J_VALUES)
    Ds = _balanced(rng, D_VALUES + D_DEEP)
    nhwc, dts = _balanced(rng, (False, True)), _balanced(rng, (F32, F16, BF16))
    odd, hws = _balanced(rng, (True, False)), _balanced(rng, tuple(MAPS))
    odd_maps = _balanced(rng, MAPS_DECODE, N_CASES // 2)     # every one of them, on the twelve odd cases
    rows = []
    for i in range(N_CASES):
        H, W = odd_maps.pop() if odd[i] else _map(rng, hws[i])
        rows.append(dict(B=Bs[i], C=0, J=_joints(rng, Ds[i], Js[i]), D=Ds[i], H=H, W=W, dtype=dts[i], nhwc=nhwc[i]))
    return rows


_GENERATORS = {'head32': _cases_head32, 'head16': _cases_head16, 'head16rt': _cases_head16rt, 'decode': _cases_decode}
_CASES = {}


def build_cases(family):
    """A fresh draw (tests/test_head_fuzz_host.py compares two)."""
    rng = random.Random(SEED + FAMILIES.index(family))
    return _finish(family, rng, _GENERATORS[family](rng))


def cases(family):
    if family not in _CASES:
        _CASES[family] = build_cases(family)
        assert len(_CASES[family]) == N_CASES
    return _CASES[family]


def case_id(c):
    dt = {F32: 'f32', F16: 'f16', BF16: 'bf16'}[c['dtype']]
    return (f"{c['index']}-b{c['B']}c{c['C']}j{c['J']}d{c['D']}-{c['H']}x{c['W']}-{dt}-{'nhwc' if c['nhwc'] else 'nchw'}"
            f"-{c['kind']}")


def head_config(c, **changes):
    kw = dict(depth=c['D'], proc_side=c['proc_side'], stride_test=c['stride'], stride_train=c['stride'],
              centered_stride=c['centered'], legacy_centered_stride_bug=c['legacy'], box_size_mm=c['box'])
    kw.update(changes)
    return cpu_ref.HeadConfig(**kw)


def n_column_blocks(c):
    return (c['H'] * c['W'] + 63) // 64


# ---- inputs

def _row3(c, j, d):
    return c['J'] + d * c['J'] + j


def _unit_rows(c, j, three_d):
    return [_row3(c, j, d) for d in range(c['D'])] if three_d else [j]


def _spike_target(c):
    """(crop, output row, position) of a spike: position 0; position H*W - 1; the last valid position of the last
    column block of crop B - 1; depth slice D - 1."""
    B, J, D, hw = c['B'], c['J'], c['D'], c['H'] * c['W']
    i = c['index']
    return {0: (0, i % J, 0),
            1: (0, _row3(c, J - 1, D // 2), hw - 1),
            2: (B - 1, J - 1, hw - 1),
            3: (B // 2, _row3(c, i % J, D - 1), hw // 2)}[c['rotation']]


def _peak_targets(c):
    """(crop, [(row, position, amplitude)] * 2): two logits of joint J - 1's volumetric unit in different column blocks
    (the first and the last; of a one-block map: the first and the last position), in depth slices 0 and D - 1 -- for
    D > 16 different tiles of the atom."""
    hw = c['H'] * c['W']
    a0, a1 = PEAKS if c['larger_first'] else PEAKS[::-1]
    return c['index'] % c['B'], [(_row3(c, c['J'] - 1, 0), min(1, hw - 1), a0), (_row3(c, c['J'] - 1, c['D'] - 1), max(hw - 2, 0), a1)]


def inputs(c):
    """CPU tensors.  Fused families: x [B,C,H,W] in the case's dtype, w [J(1+D), C] and b f32; decode: logits in the
    case's dtype."""
    g = oracle_cases.gen(c['seed'])
    B, C, J, D, H, W = (c[k] for k in 'BCJDHW')
    n_out = J * (1 + D)
    kind = c['kind']
    if c['family'] == 'decode':
        L = torch.randn(B, n_out, H, W, generator=g) * c['gain']
        flat = L.view(B, n_out, H * W)
        if kind == 'spike':
            b, r, p = _spike_target(c)
            flat[b, r, p] += c['amp']
        elif kind == 'two_peaks':
            b, peaks = _peak_targets(c)
            for r, p, a in peaks:
                flat[b, r, p] += a
        elif kind == 'level':
            flat[:, _unit_rows(c, c['index'] % J, c['level_3d'])] = 0.5
        return dict(logits=L.to(c['dtype']))
    x = torch.randn(B, C, H, W, generator=g)
    w, b = oracle_cases.default_conv_init(n_out, C, g)
    w, b = w * c['gain'], b * c['gain']
    flat = x.view(B, C, H * W)
    raise_by = lambda r, a: a * w[r] / (w[r] @ w[r])    # (before any rounding to 16 bits)
    if kind == 'spike':
        cb, r, p = _spike_target(c)
        flat[cb, :, p] += raise_by(r, c['amp'])
    elif kind == 'two_peaks':
        cb, peaks = _peak_targets(c)
        for r, p, a in peaks:
            flat[cb, :, p] += raise_by(r, a)
    elif kind == 'level':
        rows = _unit_rows(c, c['index'] % J, c['level_3d'])
        w[rows] = 0.0
        b[rows] = 0.5
    return dict(x=x.to(c['dtype']), w=w.contiguous(), b=b.contiguous())


def _carve(t, fill, nhwc=False):
    """A copy of t [B,C,H,W] inside a flat buffer filled with `fill`, GUARD elements on either side; nhwc: the copy lies
    in [B,H,W,C] order and the view is its channels_last [B,C,H,W] view -> (buffer, view)."""
    n = t.numel()
    big = torch.full((n + 2 * GUARD,), fill, dtype=t.dtype, device=t.device)
    inner = big[GUARD:GUARD + n]
    if nhwc and t.dim() == 4:
        B, C, H, W = t.shape
        view = inner.view(B, H, W, C).permute(0, 3, 1, 2)
    else:
        view = inner.view(t.shape)
    view.copy_(t)
    return big, view


def guarded_out(shape, device):
    return _carve(torch.full(shape, SENTINEL, dtype=F32, device=device), SENTINEL)


def bands_intact(big, fill=SENTINEL):
    return bool((big[:GUARD] == fill).all()) and bool((big[-GUARD:] == fill).all())


def nan_bands_intact(big):
    return bool(torch.isnan(big[:GUARD]).all()) and bool(torch.isnan(big[-GUARD:]).all())


def on_device(c, inp, device='cuda', nhwc=None, crops=None):
    """The inputs on the device; the features / logits carved from a NaN-filled buffer ('_big').  nhwc: the layout
    (default: the case's); crops: a slice of the batch."""
    nhwc = c['nhwc'] if nhwc is None else nhwc
    name = 'logits' if c['family'] == 'decode' else 'x'
    t = inp[name] if crops is None else inp[name][crops]
    dev = {k: v.to(device) for k, v in inp.items() if k != name}
    dev['_big'], dev[name] = _carve(t.to(device), float('nan'), nhwc)
    dev['nhwc'] = nhwc
    return dev


# ---- reference and bound

def logits64(c, inp):
    """The fp64 product of the operands as the kernel consumes them [B, J(1+D), H, W] (decode: the logits)."""
    if c['family'] == 'decode':
        return inp['logits'].double()
    w = oracle_cases.head_weights_as_consumed(inp['w'], c['dtype']).double()
    return torch.einsum('oc,bchw->bohw', w, inp['x'].double()) + inp['b'].double()[None, :, None, None]


def _decode64(c, L, cfg=None):
    c2d, c3d = cpu_ref.heads_from_logits(L, c['J'], cfg or head_config(c), eval_dtype=F64)
    return c2d, c3d


def reference(c, inp):
    return _decode64(c, logits64(c, inp))


def _logit_error(c, inp, L):
    if c['family'] == 'decode':
        return torch.zeros_like(L)
    w = oracle_cases.head_weights_as_consumed(inp['w'], c['dtype']).double().abs()
    mag = torch.einsum('oc,bchw->bohw', w, inp['x'].double().abs()) + inp['b'].double().abs()[None, :, None, None]
    return (c['C'] + 2) * U * mag + U * L.abs()


def _unit_terms(L, eL):
    """L, eL [B,J,Dz,H,W], one softmax unit per (b, j) -> parts 2 + 3 of the bound for (x, y, z), each [B,J], in
    heatmap units."""
    dims = (2, 3, 4)
    n = L.shape[2] * L.shape[3] * L.shape[4]
    p = cpu_ref.joint_softmax(L, dims)
    m = L.amax(dim=dims, keepdim=True)
    eps = eL.amax(dim=dims)
    eta = (EXP_A + EXP_B * (m - L)) * U + U * L.abs().amax(dim=dims, keepdim=True)
    grow = torch.expm1(eL)
    p_eta = (p * eta).sum(dim=dims)
    out = []
    for dim in (4, 3, 2):
        shape = [1] * 5
        shape[dim] = L.shape[dim]
        coord = cpu_ref.ref_linspace(0.0, 1.0, L.shape[dim], dtype=F64).reshape(shape)
        E = (p * coord).sum(dim=dims)
        through = torch.exp(eps) * (p * (coord - E[:, :, None, None, None]).abs() * grow).sum(dim=dims)
        own = (p * coord * eta).sum(dim=dims) + E * p_eta + (2 * (n + 4) + 4) * U * E
        out.append(through + own)
    return out


def bound(c, inp, ref=None):
    """(bound2d [B,J,2], bound3d [B,J,3]) on |got - reference(c, inp)| (module docstring)."""
    B, J, D, H, W = (c[k] for k in 'BJDHW')
    L = logits64(c, inp)
    eL = _logit_error(c, inp, L)
    ref2d, ref3d = ref if ref is not None else _decode64(c, L)
    x2, y2, _ = _unit_terms(L[:, :J, None], eL[:, :J, None])
    to_units = lambda t: t[:, J:].reshape(B, D, J, H, W).permute(0, 2, 1, 3, 4)
    x3, y3, z3 = _unit_terms(to_units(L), to_units(eL))
    last = c['proc_side'] - 1
    last_center = float(last - last % c['stride'])
    mm = last_center * c['box'] / c['proc_side']
    b2 = last_center * torch.stack([x2, y2], dim=-1) + 5 * U * ref2d.abs() + FLOOR * last_center
    scale3 = torch.tensor([mm, mm, c['box']], dtype=F64)
    b3 = scale3 * torch.stack([x3, y3, z3], dim=-1) + 5 * U * ref3d.abs() + FLOOR * scale3
    return b2, b3


_TRUTH = {}


def truth(c):
    """(inputs, reference, bound) of a case, computed once and shared; leave them unchanged."""
    key = (c['family'], c['index'])
    if key not in _TRUTH:
        inp = inputs(c)
        ref = reference(c, inp)
        _TRUTH[key] = (inp, ref, bound(c, inp, ref))
    return _TRUTH[key]


def ratio(got, ref, bnd):
    """max |got - ref| / bound over both outputs; inf where an output is not finite."""
    worst = 0.0
    for g, r, b in zip(got, ref, bnd):
        g = g.detach().cpu().double()
        if g.shape != r.shape or not bool(torch.isfinite(g).all()):
            return float('inf')
        err = (g - r).abs()
        # (a scale of zero -- last_center = 0 on a one-position map -- leaves a bound of zero: the output is exactly 0)
        worst = max(worst, float(torch.where(err == 0, torch.zeros_like(err), err / b).max()))
    return worst


def check(c, got, what=''):
    """Every output finite and within its bound -> err / bound (max)."""
    _, ref, bnd = truth(c)
    r = ratio(got, ref, bnd)
    assert r <= 1.0, f'{case_id(c)} {what}: err / bound = {r:.3g}'
    return r


# ---- wrong answers

WRONG = ('last_channel', 'jd_interleave', 'flip_x', 'centered', 'joint_shift', 'bias_depth', 'xy_swapped', 'last_block')
EVERY_CASE = tuple(k for k in WRONG if k != 'bias_depth')   # must be rejected on every case they apply to


def wrong_applies(kind, c):
    """Whether the mistake is a DIFFERENT function on the case -- a rule on the case, never the outcome.  (The decode
    family has no input channels and no bias: 'last_channel' and 'bias_depth' belong to the fused families.  A map one
    column wide is its own mirror image.)"""
    fused = c['family'] != 'decode'
    return {'last_channel': fused,
            'jd_interleave': c['J'] >= 2 and c['D'] >= 2,
            'flip_x': c['W'] >= 2,
            'centered': True,
            'joint_shift': c['J'] >= 2,
            'bias_depth': fused and c['D'] >= 2 and c['kind'] == 'flat',
            'xy_swapped': c['H'] != c['W'],
            'last_block': c['H'] * c['W'] > 64}[kind]


def wrong(kind, c, inp):
    """The case's answer in fp64 with one thing wrong, from the same reference function."""
    assert wrong_applies(kind, c)
    J, D, H, W = c['J'], c['D'], c['H'], c['W']
    if kind == 'last_channel':      # the last input channel left out
        return reference(c, dict(inp, x=inp['x'][:, :-1], w=inp['w'][:, :-1]))
    if kind == 'bias_depth':        # the biases of depth slices 0 and D - 1 of the last joint swapped
        b = inp['b'].clone()
        r0, r1 = _row3(c, J - 1, 0), _row3(c, J - 1, D - 1)
        b[r0], b[r1] = inp['b'][r1], inp['b'][r0]
        return reference(c, dict(inp, b=b))
    L = logits64(c, inp)
    if kind == 'centered':
        return _decode64(c, L, head_config(c, centered_stride=not c['centered']))
    if kind == 'jd_interleave':     # depth rows read as (j d) instead of (d j)
        B = L.shape[0]
        L = torch.cat([L[:, :J], L[:, J:].reshape(B, J, D, H, W).transpose(1, 2).reshape(B, D * J, H, W)], dim=1)
    elif kind == 'flip_x':
        L = L.flip(-1)
    elif kind == 'last_block':      # the positions of the last 64-position column block left out of every softmax
        L = L.clone()
        L.view(L.shape[0], L.shape[1], H * W)[:, :, 64 * (n_column_blocks(c) - 1):] = float('-inf')
    c2d, c3d = _decode64(c, L)
    if kind == 'joint_shift':       # joint j written to slot j - 1
        c2d, c3d = c2d.roll(-1, dims=1), c3d.roll(-1, dims=1)
    elif kind == 'xy_swapped':
        c2d, c3d = c2d[..., [1, 0]], c3d[..., [1, 0, 2]]
    return c2d, c3d


def oracle32(c, inp):
    """The oracle's own f32 evaluation of the case: cpu_ref.heads_forward on the operands as consumed."""
    cfg = head_config(c)
    if c['family'] == 'decode':
        return cpu_ref.heads_from_logits(inp['logits'].float(), c['J'], cfg)
    w = oracle_cases.head_weights_as_consumed(inp['w'], c['dtype'])
    return cpu_ref.heads_forward(inp['x'].float(), w, inp['b'], c['J'], cfg)


# ---- launches

def kernel_config(c):
    from metrabs_amd.config import MetrabsConfig
    return MetrabsConfig.from_any(head_config(c).as_dict())


def run(kernels, c, dev, out=None, workspace=None, nhwc_staging=0, **options):
    """The launch through metrabs_amd.kernels -> (coords2d, coords3d_rel).  dev: on_device(...)."""
    cfg = kernel_config(c)
    if c['family'] == 'decode':
        return kernels.softargmax_decode(dev['logits'], c['J'], cfg, out=out, nhwc_staging=nhwc_staging)
    if 'packed' not in dev:
        dev['packed'] = kernels.head_pack_weights(dev['w'], dev['b'], c['J'], c['D'], c['dtype'])
    return kernels.head_fused(dev['x'], dev['packed'], c['C'], c['J'], cfg, out=out, workspace=workspace, **options)


def plan(kernels, c, B=None, nhwc=None, have_workspace=True, **options):
    nhwc = c['nhwc'] if nhwc is None else nhwc
    return kernels.head_plan(c['B'] if B is None else B, c['C'], c['H'], c['W'], c['J'], c['D'], c['dtype'],
                             channels_last=nhwc, have_workspace=have_workspace, **options)


def _signature(p):
    return p['kernel'], p['tiles_per_workgroup'], p['column_blocks'], p['split_column_blocks']


def candidate_options(c):
    """The option dicts variants() draws from; 'workspace': False = the launch without one."""
    if c['family'] == 'decode':
        return []
    if c['family'] == 'head16':
        return [dict(groups_per_workgroup=g, dma_staging=s) for s in range(8) for g in (0, 1, 2, 3, 4)]
    out = [dict(rt_tiles=t) for t in range(1, 6)]
    out += [dict(rt_split=2), dict(rt_split=2, workspace=False), dict(rt_split=1)]
    out += [dict(rt_tiles=t, rt_split=2) for t in range(1, 6)]
    if c['family'] == 'head32':
        out += [dict(rt_tiles=t, rt_loader=ld, rt_split=1, rt_column_blocks=1) for ld in (1, 2) for t in range(1, 6)]
        out += [dict(rt_column_blocks=n, rt_split=1, rt_loader=1) for n in range(1, 5)]
        out += [dict(rt_column_blocks=2, rt_tiles=2, rt_split=1, rt_loader=1)]
        out += [dict(rt_k_groups=2, rt_tiles=t, rt_loader=1, rt_split=1, rt_column_blocks=1) for t in (1, 2, 3)]
        out += [dict(rt_tiles=t, rt_loader=2, rt_split=2) for t in (1, 3)]
    return out


def variants(kernels, c, nhwc=None):
    """The option dicts whose kernels.head_plan reports a kernel or tiling not yet in the list (the default's first) ->
    [(options, plan)]; the counterpart of K13.configs in conv_fuzz.py."""
    if c['family'] == 'decode':
        return []
    first = plan(kernels, c, nhwc=nhwc)
    assert first is not None, case_id(c)
    seen, out = {_signature(first)}, []
    for opts in candidate_options(c):
        kw = {k: v for k, v in opts.items() if k != 'workspace'}
        p = plan(kernels, c, nhwc=nhwc, have_workspace=opts.get('workspace', True), **kw)
        if p is None or _signature(p) in seen:
            continue
        seen.add(_signature(p))
        out.append((opts, p))
    return out

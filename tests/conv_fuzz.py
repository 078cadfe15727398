"""Seeded shape fuzz of the backbone convolution kernels (K10 .. K22): a helper of tests/test_conv_fuzz_host.py (CPU)
and tests/test_gpu_conv_fuzz.py (GPU), no test module itself.

Per kernel one adapter (KERNELS[name]) with
  * cases(): 24 cases from random.Random(a fixed seed) -- Python's generator, so the draws do not move with the torch
    version.  A case is a dict: the shape plus one choice of every optional input of the entry point (activation, gate,
    residual, in_bias with in_act, stride, padding, dtype, want_mean).  Every case lies inside the kernel's domain BY
    CONSTRUCTION: the generator multiplies the entry's divisibility rules out (a width is drawn from the widths the
    height allows, a channel count from the counts that fit the kernel's LDS) -- nothing is drawn and rejected;
  * accept(lib, case): the C entry point on host buffers with B = 0 (every entry makes its argument checks before
    "B == 0: nothing to do"), one return code per call;
  * supported(case, device, shift): the kernels.*_supported predicate where it works on tensors of that device, else None;
  * inputs(case, device, guard): the tensors, with the scaling of the kernel's own test module; guard=True carves x and
    the residual out of NaN-filled buffers;
  * check(case, inputs, got, mean) / reference(case, inputs): the `_check` and the (fp64 reference, bound) OF THE
    KERNEL'S OWN TEST MODULE -- imported, not copied; no tolerance is defined in this file;
  * wrong(case, inputs): subtly wrong fp64 references (the last input channel left out, two taps of the 3x3 swapped,
    bias[m - 1] on the last channel, the residual added before the activation) for the checker's self-test;
  * run(kernels, case, inputs, out=...): the launch through metrabs_amd.kernels; tiles(case): the workgroup's tile.
"""
import ctypes
import math
import random

import torch
import torch.nn.functional as F

N_CASES = 24
ACTS = [None, 'relu', 'silu', 'hardswish']
ACT_CODES = {None: 0, 'relu': 1, 'silu': 2, 'hardswish': 3}
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DT_CODE = {F32: 0, F16: 1, BF16: 2}
GUARD = 256          # elements on either side of a guarded tensor: its base stays 16-byte aligned
SENTINEL = -32768.0   # exact in f32, f16 and bf16, and far outside every result
_ACT64 = {None: lambda t: t, 'relu': F.relu, 'silu': F.silu, 'hardswish': F.hardswish}

# ---- host buffers for the B = 0 calls: nothing is read or written, only the pointers' values are looked at
_store = (ctypes.c_char * (1 << 12))()
_base = (ctypes.addressof(_store) + 255) & ~255


class Pointers:
    """The addresses an entry point is called with: x, y, the weights (W, W1), biases (B, B1), gate, residual, mean."""
    NAMES = ('X', 'Y', 'W', 'W1', 'B', 'B1', 'G', 'R', 'M')

    def __init__(self, base, spacing):
        for i, n in enumerate(self.NAMES):
            setattr(self, n, base + spacing * i)


HOST = Pointers(_base, 256)


def _opt(flag, ptr):
    return ptr if flag else None


# ---- draws

def _balanced(rng, values, n=N_CASES):
    """n values, every one of `values` as often as the others (to within one), in a shuffled order."""
    out = [values[i % len(values)] for i in range(n)]
    rng.shuffle(out)
    return out


def _widths(H, group, lo=1, hi=24, step=1):
    """The widths in lo .. hi (multiples of `step`) with H * W a multiple of `group`."""
    need = group // math.gcd(H, group)
    need = need * step // math.gcd(need, step)
    return [w for w in range(need, hi + 1, need) if w >= lo]


def _draw_map(rng, kind, group=1, wstep=1, hstep=1, hi=24):
    """(H, W) with H % hstep == 0, W % wstep == 0 and H * W % group == 0, drawn from the allowed values only.
    kind: 'tiny' at most 3 rows and 8 columns (fewer positions than any kernel's column tile), 'rect' H != W, 'square'
    H == W where the rules allow one, 'any'."""
    top = 3 if kind == 'tiny' else hi
    H = hstep * rng.randint(1, max(1, top // hstep))
    ws = _widths(H, group, 1, 8 if kind == 'tiny' else hi, wstep)
    if kind == 'rect':
        ws = [w for w in ws if w != H] or ws
    if kind == 'square' and H in ws:
        return H, H
    return H, rng.choice(ws)


def _cout_slots(rng, past, mult8_hi=300, odd_hi=127):
    """24 output-channel counts: 1 once, 2 .. 7 three times, six that are no multiple of 8 below one channel tile, four
    from `past` (past one workgroup's channel tile and no multiple of it) and ten multiples of 8."""
    out = [1] + [rng.randint(2, 7) for _ in range(3)]
    out += [8 * rng.randint(1, odd_hi // 8) + rng.randint(1, 7) for _ in range(6)]
    out += [rng.choice(past) for _ in range(4)]
    out += [8 * rng.randint(1, mult8_hi // 8) for _ in range(10)]
    rng.shuffle(out)
    return out


def _map_kinds(rng):
    """24 map kinds: four tiny maps (with B = 1: fewer columns than a tile), four small maps with B >= 2 (a tile spans
    two images where tiles run over images), ten rectangles, six of any shape."""
    kinds = ['tiny'] * 4 + ['span'] * 4 + ['rect'] * 10 + ['any'] * 6
    rng.shuffle(kinds)
    return kinds


def tile_spans_two_images(B, HW, bn):
    """Whether one of the bn-column tiles over the B * HW joint columns holds columns of two images."""
    n = B * HW
    return any(s // HW != (min(s + bn, n) - 1) // HW for s in range(0, n, bn))


# ---- inputs

def _gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def _carve(t, fill):
    """A copy of t inside a buffer filled with `fill`, GUARD elements on either side -> (buffer, view)."""
    n = t.numel()
    big = torch.full((n + 2 * GUARD,), fill, dtype=t.dtype, device=t.device)
    view = big[GUARD:GUARD + n].view(t.shape)
    view.copy_(t)
    return big, view


def guarded_out(shape, dtype, device):
    """(buffer, out): `out` of `shape` inside a buffer filled with SENTINEL, itself filled with it too."""
    return _carve(torch.full(shape, SENTINEL, dtype=dtype, device=device), SENTINEL)


def bands_intact(big, fill=SENTINEL):
    return bool((big[:GUARD] == fill).all()) and bool((big[-GUARD:] == fill).all())


def _nan_guard(inp, names, guard):
    if guard:
        for n in names:
            if inp.get(n) is not None:
                inp['_big_' + n], inp[n] = _carve(inp[n], float('nan'))
    return inp


def _empty(shape, dtype, device, shift=0):
    """An uninitialised contiguous tensor whose base lies `shift` bytes past a 16-byte boundary."""
    es = torch.empty(0, dtype=dtype).element_size()
    n = math.prod(shape)
    return torch.empty(n + 16, dtype=dtype, device=device)[shift // es:shift // es + n].view(shape)


def _bordered(x, border):
    H, W = x.shape[2:]
    edge = torch.ones(H, W, device=x.device)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = border
    return x * edge


class Kernel:
    name = ''
    mfma = False            # an MFMA convolution kernel: the output-channel and column-tile conditions apply
    joint_columns = False   # its column tiles run over (image, position) jointly
    has_mean = False

    def cases(self):
        if not hasattr(self, '_cases'):
            self._cases = self._generate(random.Random(self.seed))
            assert len(self._cases) == N_CASES
        return self._cases

    def supported(self, c, device='cpu', shift=0):
        """The kernels.*_supported predicate on empty tensors of the case's shapes (x `shift` bytes past a 16-byte
        boundary), or None: the kernel has none, or it asks for CUDA tensors and `device` is the CPU."""
        return None

    def wrong(self, c, inp):
        return {}

    def _residual_first(self, c, inp, out):
        if c['act'] is not None and inp.get('r') is not None:
            z, _ = self.reference(dict(c, act=None), dict(inp, r=None))
            out['residual_first'] = _ACT64[c['act']](z + inp['r'].double())


# ================================================================================================ the 1x1 family

class _Conv1x1(Kernel):
    mfma = True
    joint_columns = True
    group = 4
    dtypes = [F32]
    prologue = True
    past = [m for m in range(161, 301) if m % 64]   # past every configuration's 64- / 128-channel tile

    def _generate(self, rng):
        g = self.group
        couts, kinds = _cout_slots(rng, self.past), _map_kinds(rng)
        acts, gates, ress = _balanced(rng, ACTS), _balanced(rng, [False, True]), _balanced(rng, [False, True])
        pres, in_acts = _balanced(rng, [False, True]), _balanced(rng, ACTS)
        dts = _balanced(rng, self.dtypes)
        deep = set(rng.sample(range(N_CASES), 4))     # K of 400 .. 600: the deep-K rings wrap
        cases = []
        for i in range(N_CASES):
            H, W = _draw_map(rng, 'tiny' if kinds[i] in ('tiny', 'span') else kinds[i], group=g)
            B = 1 if kinds[i] == 'tiny' else rng.randint(2, 5) if kinds[i] == 'span' else rng.randint(1, 5)
            K = g * (rng.randint(400 // g, 600 // g) if i in deep else rng.randint(1, 300 // g))
            c = dict(B=B, K=K, M=couts[i], H=H, W=W, act=acts[i], gate=gates[i], residual=ress[i], dtype=dts[i])
            if self.prologue:
                c.update(in_bias=pres[i], in_act=in_acts[i] if pres[i] else None)
            cases.append(c)
        return cases

    def inputs(self, c, device, guard=False, seed=0):
        g = _gen(device, 1000 + seed)
        B, K, M, H, W, dt = c['B'], c['K'], c['M'], c['H'], c['W'], c['dtype']
        x = torch.randn(B, K, H, W, device=device, generator=g).to(dt)
        w = (torch.randn(M, K, 1, 1, device=device, generator=g) / K ** 0.5).to(dt)
        b = 0.5 * torch.randn(M, device=device, generator=g)
        b_in = 3.0 + 0.5 * torch.randn(K, device=device, generator=g)   # act(b_in) far from zero: a zero fill shows
        gt = torch.rand(B, K, device=device, generator=g)
        r = torch.randn(B, M, H, W, device=device, generator=g).to(dt)
        inp = dict(x=x, w=w, b=b, gate=gt if c['gate'] else None, r=r if c['residual'] else None,
                   b_in=b_in if c.get('in_bias') else None)
        return _nan_guard(inp, ('x', 'r'), guard)

    def gemm_input(self, c, inp, kernels=None):
        """What enters the GEMM: x, or with a prologue K10's result on x (on the GPU: K10's own bits)."""
        if inp['b_in'] is None:
            return inp['x']
        if kernels is not None:
            return kernels.bias_act_(inp['x'].clone(), inp['b_in'], c['in_act'])
        return _ACT64[c['in_act']](inp['x'] + inp['b_in'][None, :, None, None])

    def _args(self, c, inp):
        x = inp['x10'] if inp.get('x10') is not None else self.gemm_input(c, inp)
        return x, inp['w'], inp['b'], c['act'], inp['gate'], inp['r']

    def reference(self, c, inp):
        return self.module()._reference(*self._args(c, inp))

    def check(self, c, inp, got, mean=None):
        self.module()._check(*self._args(c, inp), got)

    def wrong(self, c, inp):
        out = {}
        cut = dict(inp, x=inp['x'][:, :-1], w=inp['w'][:, :-1], x10=None,
                   gate=None if inp['gate'] is None else inp['gate'][:, :-1],
                   b_in=None if inp['b_in'] is None else inp['b_in'][:-1])
        out['last_channel'] = self.reference(c, cut)[0]
        if c['M'] >= 2:
            b = inp['b'].clone()
            b[-1] = inp['b'][-2]
            out['bias_shift'] = self.reference(c, dict(inp, b=b))[0]
        self._residual_first(c, inp, out)
        return out

    def out_shape(self, c):
        return (c['B'], c['M'], c['H'], c['W'])


class K13(_Conv1x1):
    name, seed = 'k13', 1301
    CONFIGS = ['wide', 'square', 'tall', 'deepk', 'stream', 'deep64']

    def module(self):
        import test_gpu_conv1x1
        return test_gpu_conv1x1

    def configs(self, kernels, c):
        """'auto' and every named configuration that conv1x1_plan resolves to itself for the shape."""
        HW = c['H'] * c['W']
        return ['auto'] + [n for n in self.CONFIGS if kernels.conv1x1_plan(c['M'], c['K'], HW, c['B'], n)[0] == n]

    def tiles(self, kernels, c):
        _, _, bm, bn = kernels.conv1x1_plan(c['M'], c['K'], c['H'] * c['W'], c['B'])
        return bm, bn

    def accept(self, lib, c, B=0, p=None):
        p = p or HOST
        from metrabs_amd import kernels
        return [lib.mtr_conv1x1_bias_act_pre(
            p.X, 0, p.W, p.B, _opt(c['in_bias'], p.B1), ACT_CODES[c['in_act']], _opt(c['gate'], p.G),
            _opt(c['residual'], p.R), ACT_CODES[c['act']], B, c['M'], c['K'], c['H'] * c['W'], p.Y, None,
            kernels.CONV1X1_CONFIGS[cfg]) for cfg in self.configs(kernels, c)]

    def supported(self, c, device='cpu', shift=0):
        from metrabs_amd import kernels
        return kernels.conv1x1_supported(_empty((c['B'], c['K'], c['H'], c['W']), F32, device, shift),
                                         _empty((c['M'], c['K']), F32, device))

    def run(self, kernels, c, inp, out=None, config='auto', prologue=True):
        if prologue:
            return kernels.conv1x1_bias_act(inp['x'], inp['w'], inp['b'], c['act'], gate=inp['gate'], residual=inp['r'],
                                            out=out, config=config, in_bias=inp['b_in'], in_act=c['in_act'])
        return kernels.conv1x1_bias_act(inp['x10'], inp['w'], inp['b'], c['act'], gate=inp['gate'], residual=inp['r'],
                                        out=out, config=config)


class K13h(_Conv1x1):
    name, seed = 'k13h', 1316
    group = 8
    dtypes = [F16, BF16]
    prologue = False
    CONFIGS = ['tall', 'square', 'deepk']

    def module(self):
        import test_gpu_backbone16
        return test_gpu_backbone16

    def configs(self, kernels, c):
        HW = c['H'] * c['W']
        return ['auto'] + [n for n in self.CONFIGS if kernels.conv1x1_16_plan(c['M'], c['K'], HW, c['B'], n)[0] == n]

    def tiles(self, kernels, c):
        _, _, bm, bn = kernels.conv1x1_16_plan(c['M'], c['K'], c['H'] * c['W'], c['B'])
        return bm, bn

    def accept(self, lib, c, B=0, p=None):
        p = p or HOST
        from metrabs_amd import kernels
        return [lib.mtr_conv1x1_bias_act16_opts(
            p.X, DT_CODE[c['dtype']], p.W, p.B, _opt(c['gate'], p.G), _opt(c['residual'], p.R), ACT_CODES[c['act']], B,
            c['M'], c['K'], c['H'] * c['W'], p.Y, None, kernels.CONV1X1_16_CONFIGS[cfg])
            for cfg in self.configs(kernels, c)]

    def supported(self, c, device='cpu', shift=0):
        from metrabs_amd import kernels
        return kernels.conv1x1_16_supported(_empty((c['B'], c['K'], c['H'], c['W']), c['dtype'], device, shift),
                                            _empty((c['M'], c['K']), c['dtype'], device))

    def run(self, kernels, c, inp, out=None, config='auto'):
        return kernels.conv1x1_bias_act16(inp['x'], inp['w'], inp['b'], c['act'], gate=inp['gate'], residual=inp['r'],
                                          out=out, config=config)


def split_tiles_per_wave(M, n_total):
    """split_tiles_per_wave of csrc/conv1x1_split.hip, restated: 16-channel tiles per wave of K20's workgroup."""
    n_mt, gx = (M + 15) // 16, (n_total + 63) // 64
    mt = min((n_mt + 3) // 4, 4)
    while mt > 1 and gx * ((n_mt + 4 * mt - 1) // (4 * mt)) < 256:
        mt -= 1
    return mt


class K20(_Conv1x1):
    name, seed = 'k20', 2001

    def module(self):
        import test_gpu_conv1x1_split
        return test_gpu_conv1x1_split

    def tiles(self, kernels, c):
        return 64 * split_tiles_per_wave(c['M'], c['B'] * c['H'] * c['W']), 64

    def accept(self, lib, c, B=0, p=None):
        p = p or HOST
        return [lib.mtr_conv1x1_bias_act_split(
            p.X, p.W, p.B, _opt(c['in_bias'], p.B1), ACT_CODES[c['in_act']], _opt(c['gate'], p.G),
            _opt(c['residual'], p.R), ACT_CODES[c['act']], B, c['M'], c['K'], c['H'] * c['W'], p.Y, None),
            lib.mtr_conv1x1_split_supported(B, c['M'], c['K'], c['H'] * c['W'])]

    def supported(self, c, device='cpu', shift=0):
        from metrabs_amd import kernels
        if device == 'cpu':
            return None
        return kernels.conv1x1_split_supported(_empty((c['B'], c['K'], c['H'], c['W']), F32, device, shift),
                                               _empty((3, c['M'], (c['K'] + 31) // 32 * 32), BF16, device))

    def run(self, kernels, c, inp, out=None, prologue=True):
        ws = kernels.pack_conv1x1_split_weight(inp['w'])
        assert kernels.conv1x1_split_supported(inp['x'], ws), c
        if prologue:
            return kernels.conv1x1_bias_act_split(inp['x'], ws, inp['b'], c['act'], gate=inp['gate'], residual=inp['r'],
                                                  in_bias=inp['b_in'], in_act=c['in_act'], out=out)
        return kernels.conv1x1_bias_act_split(inp['x10'], ws, inp['b'], c['act'], gate=inp['gate'], residual=inp['r'],
                                              out=out)


# ================================================================================================ the dense 3x3 family

def halo_positions(Ho, Wo, stride, BN):
    """conv3x3_geometry of csrc/conv3x3_16.hip (and fmb_geometry), restated: the staged halo's rows x columns for the
    tile width in {64, 32, 16, 8} that pads the output map least (the wider one on a tie)."""
    best = lw = None
    for cand in (6, 5, 4, 3):
        TW, TH = 1 << cand, BN >> cand
        padded = -(-Wo // TW) * TW * (-(-Ho // TH) * TH)
        if best is None or padded < best:
            best, lw = padded, cand
    TW, TH = 1 << lw, BN >> lw
    return ((TH - 1) * stride + 3) * (4 * (((TW - 1) * stride + 9) // 4))


def cins_within_lds(positions, budget, hi=296):
    """The input-channel counts (multiples of 8 up to hi) whose halo of `positions` x LDC 16-bit elements fits `budget`
    bytes; LDC = Cin, or Cin + 8 where Cin is a multiple of 16."""
    return [k for k in range(8, hi + 1, 8) if positions * (k + (0 if k & 8 else 8)) * 2 <= budget]


def k14h_channel_tile(M):
    """launch_conv3x3_16's table: (channels, positions) of a workgroup's tile."""
    if M <= 32:
        return 32, 256
    if M <= 96:
        return 96, 128
    return (192, 128) if (128 < M <= 192 or M % 192 == 0) else (128, 128)


class _Conv3x3(Kernel):
    mfma = True

    def _epilogues(self, rng):
        return _balanced(rng, ACTS), _balanced(rng, [False, True])

    def inputs(self, c, device, guard=False, seed=0):
        g = _gen(device, 2000 + seed)
        B, K, M, H, W, dt, s = c['B'], c['K'], c['M'], c['H'], c['W'], c['dtype'], c['stride']
        x = _bordered(torch.randn(B, K, H, W, device=device, generator=g), 8.0).to(dt)
        w = (torch.randn(M, K, 3, 3, device=device, generator=g) / (9 * K) ** 0.5).to(dt)
        b = 0.5 * torch.randn(M, device=device, generator=g)
        r = torch.randn(B, M, (H - 1) // s + 1, (W - 1) // s + 1, device=device, generator=g).to(dt)
        return _nan_guard(dict(x=x, w=w, b=b, r=r if c['residual'] else None), ('x', 'r'), guard)

    def check(self, c, inp, got, mean=None):
        self.module()._check(*self._args(c, inp), got)

    def reference(self, c, inp):
        return self.module()._reference(*self._args(c, inp))

    def wrong(self, c, inp):
        out = {'last_channel': self.reference(c, dict(inp, x=inp['x'][:, :-1], w=inp['w'][:, :-1]))[0]}
        w = inp['w'].clone()
        w[:, :, 0, 1], w[:, :, 1, 0] = inp['w'][:, :, 1, 0], inp['w'][:, :, 0, 1]
        out['taps_swapped'] = self.reference(c, dict(inp, w=w))[0]
        if c['M'] >= 2:
            b = inp['b'].clone()
            b[-1] = inp['b'][-2]
            out['bias_shift'] = self.reference(c, dict(inp, b=b))[0]
        self._residual_first(c, inp, out)
        return out

    def out_shape(self, c):
        s = c['stride']
        return (c['B'], c['M'], (c['H'] - 1) // s + 1, (c['W'] - 1) // s + 1)


class K14h(_Conv3x3):
    name, seed = 'k14h', 1416
    past = [m for m in range(193, 301) if m % 128]   # 128-channel tiles there (192-channel ones end at 192)

    def module(self):
        import test_gpu_conv3x3_16
        return test_gpu_conv3x3_16

    def _generate(self, rng):
        couts, kinds = _cout_slots(rng, self.past), _map_kinds(rng)
        (acts, ress), strides = self._epilogues(rng), _balanced(rng, [1, 2])
        dts = _balanced(rng, [F16, BF16])
        cases = []
        for i in range(N_CASES):
            s, M = strides[i], couts[i]
            # W % 4 == 0 and Wo % 4 == 0: at stride 2 W is a multiple of 8
            H, W = _draw_map(rng, 'tiny' if kinds[i] in ('tiny', 'span') else kinds[i], wstep=4 * s)
            Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
            K = rng.choice(cins_within_lds(halo_positions(Ho, Wo, s, k14h_channel_tile(M)[1]), 160 * 1024))
            cases.append(dict(B=1 if kinds[i] == 'tiny' else rng.randint(1, 5), K=K, M=M, H=H, W=W, stride=s,
                              act=acts[i], residual=ress[i], dtype=dts[i]))
        return cases

    def tiles(self, kernels, c):
        return k14h_channel_tile(c['M'])

    def _args(self, c, inp):
        return inp['x'], inp['w'], inp['b'], c['act'], c['stride'], inp['r']

    def accept(self, lib, c, B=0, p=None):
        p = p or HOST
        return [lib.mtr_conv3x3_bias_act16(p.X, DT_CODE[c['dtype']], p.W, p.B, _opt(c['residual'], p.R),
                                           ACT_CODES[c['act']], B, c['K'], c['M'], c['H'], c['W'], c['stride'], p.Y, None)]

    def supported(self, c, device='cpu', shift=0):
        from metrabs_amd import kernels
        return kernels.conv3x3_16_supported(_empty((c['B'], c['K'], c['H'], c['W']), c['dtype'], device, shift),
                                            _empty((c['M'], 3, 3, c['K']), c['dtype'], device), c['stride'])

    def run(self, kernels, c, inp, out=None):
        wp = kernels.pack_conv3x3_weight(inp['w'])
        assert kernels.conv3x3_16_supported(inp['x'], wp, c['stride']), c
        return kernels.conv3x3_bias_act16(inp['x'], wp, inp['b'], c['act'], c['stride'], residual=inp['r'], out=out)


class K19(_Conv3x3):
    name, seed = 'k19', 1901
    joint_columns = True
    past = [m for m in range(33, 301) if m % 32]   # 32 output channels per workgroup

    def module(self):
        import test_gpu_conv3x3_winograd
        return test_gpu_conv3x3_winograd

    def _generate(self, rng):
        couts, kinds = _cout_slots(rng, self.past, odd_hi=31), _map_kinds(rng)
        acts, ress = self._epilogues(rng)
        cases = []
        for i in range(N_CASES):
            H, W = _draw_map(rng, 'tiny' if kinds[i] in ('tiny', 'span') else kinds[i], wstep=4, hstep=2)
            B = 1 if kinds[i] == 'tiny' else rng.randint(2, 5) if kinds[i] == 'span' else rng.randint(1, 5)
            cases.append(dict(B=B, K=4 * rng.randint(1, 75), M=couts[i], H=H, W=W, stride=1, act=acts[i],
                              residual=ress[i], dtype=F32))
        return cases

    def tiles(self, kernels, c):
        return 32, 256   # 64 Winograd tiles of 2 x 2 outputs, over image and position jointly

    def _args(self, c, inp):
        return inp['x'], inp['w'], inp['b'], c['act'], inp['r']

    def accept(self, lib, c, B=0, p=None):
        p = p or HOST
        return [lib.mtr_conv3x3_winograd_bias_act(p.X, p.W, p.B, _opt(c['residual'], p.R), ACT_CODES[c['act']], B,
                                                  c['K'], c['M'], c['H'], c['W'], p.Y, None),
                0 if lib.mtr_conv3x3_winograd_lds_bytes(c['B'], c['K'], c['M'], c['H'], c['W']) > 0 else -2]

    def supported(self, c, device='cpu', shift=0):
        from metrabs_amd import kernels
        if device == 'cpu':
            return None
        return kernels.conv3x3_winograd_supported(_empty((c['B'], c['K'], c['H'], c['W']), F32, device, shift),
                                                  _empty((16, c['M'], c['K']), F32, device))

    def run(self, kernels, c, inp, out=None):
        wu = kernels.pack_conv3x3_winograd_weight(inp['w'])
        assert kernels.conv3x3_winograd_supported(inp['x'], wu), c
        return kernels.conv3x3_winograd_bias_act(inp['x'], wu, inp['b'], c['act'], residual=inp['r'], out=out)


def k22_channel_block(M):
    """conv3x3s2_shape's channel block: ceil(M / 128) equal blocks, rounded up to 16 channels."""
    m_blocks = (M + 127) // 128
    return ((M + m_blocks - 1) // m_blocks + 15) // 16 * 16


class K22(_Conv3x3):
    name, seed = 'k22', 2201
    past = [m for m in range(129, 301) if m % k22_channel_block(m)]

    def module(self):
        import test_gpu_conv3x3_strided
        return test_gpu_conv3x3_strided

    def _generate(self, rng):
        couts, kinds = _cout_slots(rng, self.past), _map_kinds(rng)
        acts, ress = self._epilogues(rng)
        cases = []
        for i in range(N_CASES):
            H, W = _draw_map(rng, 'tiny' if kinds[i] in ('tiny', 'span') else kinds[i], wstep=8, hstep=2)
            cases.append(dict(B=1 if kinds[i] == 'tiny' else rng.randint(1, 5), K=4 * rng.randint(1, 75), M=couts[i],
                              H=H, W=W, stride=2, act=acts[i], residual=ress[i], dtype=F32))
        return cases

    def tiles(self, kernels, c):
        return k22_channel_block(c['M']), 128

    def _args(self, c, inp):
        return inp['x'], inp['w'], inp['b'], c['act'], inp['r']

    def accept(self, lib, c, B=0, p=None):
        p = p or HOST
        return [lib.mtr_conv3x3s2_bias_act(p.X, p.W, p.B, _opt(c['residual'], p.R), ACT_CODES[c['act']], B, c['K'],
                                           c['M'], c['H'], c['W'], p.Y, None),
                0 if lib.mtr_conv3x3s2_lds_bytes(c['B'], c['K'], c['M'], c['H'], c['W']) > 0 else -2]

    def supported(self, c, device='cpu', shift=0):
        from metrabs_amd import kernels
        if device == 'cpu':
            return None
        return kernels.conv3x3_strided_supported(_empty((c['B'], c['K'], c['H'], c['W']), F32, device, shift),
                                                 _empty((max(c['K'] // 4, 1), c['M'], 3, 3, 4), F32, device))

    def run(self, kernels, c, inp, out=None):
        wp = kernels.pack_conv3x3_strided_weight(inp['w'])
        assert kernels.conv3x3_strided_supported(inp['x'], wp), c
        return kernels.conv3x3_strided_bias_act(inp['x'], wp, inp['b'], c['act'], residual=inp['r'], out=out)


# ================================================================================================ K16h

def k16h_chunk(Cmid):
    """launch_fused_mbconv16's chunk of Cmid: 192 channels where that pads Cmid no more than 128 does."""
    return 192 if (Cmid + 191) // 192 * 192 <= (Cmid + 127) // 128 * 128 else 128


class K16h(Kernel):
    """M is Cout (at most 128: one workgroup holds all of it), so "past one workgroup's channel tile" is asked of
    Cmid and its chunk.  With a residual Cout == Cin, a multiple of 8."""
    name, seed = 'k16h', 1616
    mfma = True

    def module(self):
        import test_gpu_fused_mbconv16
        return test_gpu_fused_mbconv16

    def _generate(self, rng):
        kinds = _map_kinds(rng)
        acts, strides, dts = _balanced(rng, ACTS), _balanced(rng, [1, 2]), _balanced(rng, [F16, BF16])
        couts = [1] + [rng.randint(2, 7) for _ in range(3)] + [8 * rng.randint(1, 15) + rng.randint(1, 7) for _ in range(8)]
        couts += [8 * rng.randint(1, 16) for _ in range(4)]   # 16 without a residual ...
        rng.shuffle(couts)
        # ... and 8 with one (stride 1, Cout == Cin), half of them the input itself
        ress = [None] * 16 + ['x'] * 4 + ['other'] * 4
        rng.shuffle(ress)
        cmids = [rng.choice([m for m in range(136, 601, 8) if m > k16h_chunk(m) and m % k16h_chunk(m)])
                 for _ in range(6)]
        cmids += [8 * rng.randint(1, 48) for _ in range(18)]
        rng.shuffle(cmids)
        cases, free = [], iter(couts)
        for i in range(N_CASES):
            s = 1 if ress[i] else strides[i]
            H, W = _draw_map(rng, 'tiny' if kinds[i] in ('tiny', 'span') else kinds[i], wstep=4 * s)
            Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
            Cmid = cmids[i]
            budget = 160 * 1024 - 128 * (k16h_chunk(Cmid) + 8) * 2
            cins = cins_within_lds(halo_positions(Ho, Wo, s, 128), budget, hi=128 if ress[i] else 296)
            K = rng.choice(cins)
            cases.append(dict(B=1 if kinds[i] == 'tiny' else rng.randint(1, 5), K=K, Cmid=Cmid,
                              M=K if ress[i] else next(free), H=H, W=W, stride=s, act=acts[i], residual=ress[i],
                              dtype=dts[i], chain=(Ho * Wo) % 8 == 0))
        return cases

    def tiles(self, kernels, c):
        return k16h_chunk(c['Cmid']), 128

    def inputs(self, c, device, guard=False, seed=0):
        g = _gen(device, 3000 + seed)
        B, K, Cmid, M, H, W, dt = c['B'], c['K'], c['Cmid'], c['M'], c['H'], c['W'], c['dtype']
        x = _bordered(torch.randn(B, K, H, W, device=device, generator=g), 8.0).to(dt)
        w3 = (torch.randn(Cmid, K, 3, 3, device=device, generator=g) / (9 * K) ** 0.5).to(dt)
        b3 = 0.5 * torch.randn(Cmid, device=device, generator=g)
        w1 = (torch.randn(M, Cmid, device=device, generator=g) / Cmid ** 0.5).to(dt)
        b1 = 0.5 * torch.randn(M, device=device, generator=g)
        other = torch.randn(B, K, H, W, device=device, generator=g).to(dt)
        inp = _nan_guard(dict(x=x, w=w3, b=b3, w1=w1, b1=b1, r=other if c['residual'] == 'other' else None),
                         ('x', 'r'), guard)
        if c['residual'] == 'x':
            inp['r'] = inp['x']
        return inp

    def _args(self, c, inp):
        return inp['x'], inp['w'], inp['b'], c['act'], c['stride'], inp['w1'], inp['b1'], inp['r']

    def reference(self, c, inp):
        return self.module()._reference(*self._args(c, inp))

    def check(self, c, inp, got, mean=None):
        self.module()._check_fp64(*self._args(c, inp), got, 'fuzz')

    def wrong(self, c, inp):
        out = {'last_channel': self.reference(c, dict(inp, x=inp['x'][:, :-1], w=inp['w'][:, :-1]))[0]}
        w = inp['w'].clone()
        w[:, :, 0, 1], w[:, :, 1, 0] = inp['w'][:, :, 1, 0], inp['w'][:, :, 0, 1]
        out['taps_swapped'] = self.reference(c, dict(inp, w=w))[0]
        if c['M'] >= 2:
            b1 = inp['b1'].clone()
            b1[-1] = inp['b1'][-2]
            out['bias_shift'] = self.reference(c, dict(inp, b1=b1))[0]
        return out   # (no activation behind the project: nothing for the skip to come in front of)

    def out_shape(self, c):
        s = c['stride']
        return (c['B'], c['M'], (c['H'] - 1) // s + 1, (c['W'] - 1) // s + 1)

    def accept(self, lib, c, B=0, p=None):
        p = p or HOST
        return [lib.mtr_fused_mbconv16(p.X, DT_CODE[c['dtype']], p.W, p.B, ACT_CODES[c['act']], p.W1, p.B1,
                                       _opt(c['residual'], p.X if c['residual'] == 'x' else p.R), B, c['K'], c['Cmid'],
                                       c['M'], c['H'], c['W'], c['stride'], p.Y, None)]

    def supported(self, c, device='cpu', shift=0):
        from metrabs_amd import kernels
        dt = c['dtype']
        return kernels.fused_mbconv16_supported(_empty((c['B'], c['K'], c['H'], c['W']), dt, device, shift),
                                                _empty((c['Cmid'], 3, 3, c['K']), dt, device),
                                                _empty((c['M'], c['Cmid']), dt, device), c['stride'])

    def run(self, kernels, c, inp, out=None, chain=False):
        w3p = kernels.pack_conv3x3_weight(inp['w'])
        if chain:   # the two kernels the block replaces
            mid = kernels.conv3x3_bias_act16(inp['x'], w3p, inp['b'], c['act'], c['stride'])
            return kernels.conv1x1_bias_act16(mid, inp['w1'], inp['b1'], None, residual=inp['r'])
        assert kernels.fused_mbconv16_supported(inp['x'], w3p, inp['w1'], c['stride']), c
        return kernels.fused_mbconv16(inp['x'], w3p, inp['b'], c['act'], c['stride'], inp['w1'], inp['b1'],
                                      residual=inp['r'], out=out)


# ================================================================================================ K17, the stem

def stem_band_rows(Wo):
    """stem_band_rows of csrc/stem_conv.hip, restated (as tests/test_gpu_stem_conv.py does)."""
    th = 1
    while 2 * th <= min(32, max(1, 1024 // Wo)):
        th *= 2
    return th


class K17(Kernel):
    """Cin = 3 and Cout a multiple of 8 up to 64 are the entry's rules: the output-channel conditions do not apply."""
    name, seed = 'k17', 1701
    PAIRS = [(F32, F32), (F16, F16), (BF16, BF16), (F32, F16), (F32, BF16)]

    def module(self):
        import test_gpu_stem_conv
        return test_gpu_stem_conv

    def _generate(self, rng):
        kinds, acts, pairs = _map_kinds(rng), _balanced(rng, ACTS), _balanced(rng, self.PAIRS)
        pre, inter = _balanced(rng, [False, True]), _balanced(rng, [False, True])
        cases = []
        for i in range(N_CASES):
            H, W = _draw_map(rng, 'tiny' if kinds[i] in ('tiny', 'span') else kinds[i], wstep=8, hstep=2, hi=48)
            cases.append(dict(B=rng.randint(1, 5), K=3, M=8 * rng.randint(1, 8), H=H, W=W, stride=2, act=acts[i],
                              xdtype=pairs[i][0], dtype=pairs[i][1], preproc=pre[i], interleaved=inter[i]))
        return cases

    def inputs(self, c, device, guard=False, seed=0):
        g = _gen(device, 4000 + seed)
        B, M, H, W = c['B'], c['M'], c['H'], c['W']
        x = torch.rand(B, 3, H, W, device=device, generator=g) if c['preproc'] else \
            torch.randn(B, 3, H, W, device=device, generator=g)
        w = (torch.randn(M, 3, 3, 3, device=device, generator=g) / 27 ** 0.5).to(c['dtype'])
        b = 0.5 * torch.randn(M, device=device, generator=g)
        x = x.to(c['xdtype'])
        if c['interleaved']:   # the same values over [B, H, W, 3] memory
            x = x.permute(0, 2, 3, 1).contiguous()
            if guard:
                big, x = _carve(x, float('nan'))
            return dict(x=x.permute(0, 3, 1, 2), w=w, b=b, **({'_big_x': big} if guard else {}))
        return _nan_guard(dict(x=x, w=w, b=b), ('x',), guard)

    def reference(self, c, inp):
        m = self.module()
        z, s = m._reference(m._torch_p(inp['x'], c['dtype'], c['preproc']), inp['w'], inp['b'])
        return m._bound(z, s, c['act'], c['dtype'])

    def check(self, c, inp, got, mean=None):
        m = self.module()
        z, s = m._reference(m._torch_p(inp['x'], c['dtype'], c['preproc']), inp['w'], inp['b'])
        m._check(z, s, c['act'], got, c['dtype'], 'fuzz', [0.0])

    def wrong(self, c, inp):
        out = {'last_channel': self.reference(c, dict(inp, x=inp['x'][:, :-1], w=inp['w'][:, :-1]))[0]}
        w = inp['w'].clone()
        w[:, :, 0, 1], w[:, :, 1, 0] = inp['w'][:, :, 1, 0], inp['w'][:, :, 0, 1]
        out['taps_swapped'] = self.reference(c, dict(inp, w=w))[0]
        b = inp['b'].clone()
        b[-1] = inp['b'][-2]
        out['bias_shift'] = self.reference(c, dict(inp, b=b))[0]
        return out

    def out_shape(self, c):
        return (c['B'], c['M'], c['H'] // 2, c['W'] // 2)

    def accept(self, lib, c, B=0, p=None):
        p = p or HOST
        return [lib.mtr_stem_conv3x3s2(p.X, DT_CODE[c['xdtype']], int(c['interleaved']), p.W, p.B, DT_CODE[c['dtype']],
                                       ACT_CODES[c['act']], int(c['preproc']), B, 3, c['M'], c['H'], c['W'], p.Y, None),
                0 if lib.mtr_stem_conv_lds_bytes(DT_CODE[c['dtype']], c['B'], 3, c['M'], c['H'], c['W']) > 0 else -2]

    def supported(self, c, device='cpu', shift=0):
        from metrabs_amd import kernels
        if device == 'cpu':
            return None
        x = _empty((c['B'], c['H'], c['W'], 3) if c['interleaved'] else (c['B'], 3, c['H'], c['W']), c['xdtype'], device,
                   shift)
        return kernels.stem_conv_supported(x.permute(0, 3, 1, 2) if c['interleaved'] else x,
                                           _empty((c['M'], 3, 3, 3), c['dtype'], device))

    def run(self, kernels, c, inp, out=None):
        assert kernels.stem_conv_supported(inp['x'], inp['w']), c
        return kernels.stem_conv_bias_act(inp['x'], inp['w'], inp['b'], c['act'], preproc=c['preproc'], out=out)


# ================================================================================================ the depthwise kernels

def _channel_slots(rng, hi=300):
    """24 channel counts: 1 three times, nine odd ones, twelve of any parity."""
    out = [1] * 3 + [2 * rng.randint(1, hi // 2 - 1) + 1 for _ in range(9)] + [rng.randint(2, hi) for _ in range(12)]
    rng.shuffle(out)
    return out


def _planes(rng, ksize, stride, pad, hi=24):
    """(H, W) with an output width that is a multiple of 4 (the depthwise entries' rule) and at least one output row:
    OW = (W + pl + pr - k) // stride + 1."""
    pl, pr, pt, pb = pad
    ws = [w for w in range(1, hi + 1) if w + pl + pr >= ksize and ((w + pl + pr - ksize) // stride + 1) % 4 == 0]
    hs = [h for h in range(1, hi + 1) if h + pt + pb >= ksize]
    return rng.choice(hs), rng.choice(ws)


class _Depthwise(Kernel):
    has_mean = True
    ksize, wscale = 3, 0.4

    def inputs(self, c, device, guard=False, seed=0):
        g = _gen(device, 5000 + seed)
        B, C, H, W, k = c['B'], c['C'], c['H'], c['W'], self.ksize
        x = torch.randn(B, C, H, W, device=device, generator=g).to(c['dtype'])   # rounded to the tensor dtype first
        w = torch.randn(C, 1, k, k, device=device, generator=g) * self.wscale
        b = torch.randn(C, device=device, generator=g)
        return _nan_guard(dict(x=x, w=w, b=b), ('x',), guard)

    def wrong(self, c, inp):
        w = inp['w'].clone()
        w[:, :, 0, 1], w[:, :, 1, 0] = inp['w'][:, :, 1, 0], inp['w'][:, :, 0, 1]
        out = {'taps_swapped': self.reference(c, dict(inp, w=w))[0]}
        if c['C'] >= 2:
            b = inp['b'].clone()
            b[-1] = inp['b'][-2]
            out['bias_shift'] = self.reference(c, dict(inp, b=b))[0]
        return out

    def out_shape(self, c):
        pl, pr, pt, pb = c['pad']
        s, k = c['stride'], self.ksize
        return (c['B'], c['C'], (c['H'] + pt + pb - k) // s + 1, (c['W'] + pl + pr - k) // s + 1)


class K11(_Depthwise):
    """Every path of launch_depthwise: the stride-1 block kernel (4 x 4 .. planes of power-of-two blocks), vector and
    scalar rows at either stride, each padding variant the folded networks use."""
    name, seed = 'k11', 1101
    # (stride, (left, right, top, bottom)): symmetric 1, none, and the explicit ZeroPad2d variants in front of the
    # stride-2 layers (and their stride-1 use in the scalar rows)
    VARIANTS = [(1, (1, 1, 1, 1)), (1, (0, 0, 0, 0)), (1, (0, 2, 1, 1)), (2, (1, 1, 1, 1)), (2, (0, 1, 0, 1)),
                (2, (0, 2, 0, 2)), (2, (1, 0, 1, 0)), (2, (0, 0, 0, 0))]

    def module(self):
        import test_gpu_depthwise3x3
        return test_gpu_depthwise3x3

    def _generate(self, rng):
        chans, acts, dts = _channel_slots(rng), _balanced(rng, ACTS), _balanced(rng, [F32, F16, BF16])
        variants, means = _balanced(rng, self.VARIANTS), _balanced(rng, [False, True])
        block = set(rng.sample([i for i in range(N_CASES) if variants[i] == self.VARIANTS[0]], 2))
        cases = []
        for i in range(N_CASES):
            s, pad = variants[i]
            if i in block:   # a plane the stride-1 block kernel takes: H / 4 and W / 4 powers of two
                H, W = rng.choice([(4, 4), (8, 4), (4, 16), (8, 8), (16, 16), (16, 8)])
            else:
                H, W = _planes(rng, 3, s, pad)
            cases.append(dict(B=rng.randint(1, 5), C=chans[i], H=H, W=W, stride=s, pad=pad, act=acts[i], dtype=dts[i],
                              want_mean=means[i]))
        return cases

    def reference(self, c, inp):
        return self.module()._ref_and_bound(inp['x'], inp['w'], inp['b'], c['act'], c['stride'], c['pad'])

    def check(self, c, inp, got, mean=None):
        self.module()._check(inp['x'], inp['w'], inp['b'], c['act'], c['stride'], c['pad'], [(got, mean)], tag='fuzz')

    def accept(self, lib, c, B=0, p=None):
        p = p or HOST
        pl, pr, pt, pb = c['pad']
        return [lib.mtr_depthwise3x3_bias_act_padded(p.X, DT_CODE[c['dtype']], p.W, p.B, ACT_CODES[c['act']], B, c['C'],
                                                     c['H'], c['W'], c['stride'], pt, pl, pb, pr, p.Y,
                                                     _opt(c['want_mean'], p.M), None)]

    def run(self, kernels, c, inp, out=None):
        return kernels.depthwise3x3_bias_act(inp['x'], inp['w'], inp['b'], c['act'], c['stride'], c['pad'],
                                             want_mean=c['want_mean'])


class K15(_Depthwise):
    name, seed = 'k15', 1501
    ksize, wscale = 5, 0.3
    VARIANTS = [(1, (2, 2, 2, 2)), (2, (2, 2, 2, 2)), (2, (1, 2, 1, 2)), (2, (1, 3, 1, 3)), (1, (0, 0, 0, 0)),
                (2, (2, 1, 2, 1))]

    def module(self):
        import test_gpu_depthwise5x5
        return test_gpu_depthwise5x5

    def _generate(self, rng):
        chans, acts, dts = _channel_slots(rng), _balanced(rng, ACTS), _balanced(rng, [F32, F16, BF16])
        variants, means = _balanced(rng, self.VARIANTS), _balanced(rng, [False, True])
        cases = []
        for i in range(N_CASES):
            s, pad = variants[i]
            H, W = _planes(rng, 5, s, pad)
            cases.append(dict(B=rng.randint(1, 5), C=chans[i], H=H, W=W, stride=s, pad=pad, act=acts[i], dtype=dts[i],
                              want_mean=means[i]))
        return cases

    def reference(self, c, inp):
        return self.module()._ref_and_bound(inp['x'], inp['w'], inp['b'], c['act'], c['stride'], c['pad'])

    def check(self, c, inp, got, mean=None):
        self.module()._check(inp['x'], inp['w'], inp['b'], c['act'], c['stride'], c['pad'], got, mean, tag='fuzz')

    def accept(self, lib, c, B=0, p=None):
        p = p or HOST
        pl, pr, pt, pb = c['pad']
        return [lib.mtr_depthwise5x5_bias_act_padded(p.X, DT_CODE[c['dtype']], p.W, p.B, ACT_CODES[c['act']], B, c['C'],
                                                     c['H'], c['W'], c['stride'], pt, pl, pb, pr, p.Y,
                                                     _opt(c['want_mean'], p.M), None)]

    def supported(self, c, device='cpu', shift=0):
        from metrabs_amd import kernels
        return kernels.depthwise5x5_supported(c['H'], c['W'], c['pad'])

    def run(self, kernels, c, inp, out=None):
        return kernels.depthwise5x5_bias_act(inp['x'], inp['w'], inp['b'], c['act'], c['stride'], c['pad'],
                                             want_mean=c['want_mean'])


class K18(_Depthwise):
    """Stride 1 and padding 1 are the entry's rules, W a multiple of 4 up to 128: both strides do not apply."""
    name, seed = 'k18', 1801

    def module(self):
        import test_gpu_depthwise3x3_blocks
        return test_gpu_depthwise3x3_blocks

    def _generate(self, rng):
        chans, acts, dts = _channel_slots(rng), _balanced(rng, ACTS), _balanced(rng, [F32, F16, BF16])
        means, cols = _balanced(rng, [False, True]), _balanced(rng, [None, 4, 8])
        cases = []
        for i in range(N_CASES):
            H = rng.randint(1, 24)
            eight = cols[i] == 8 and dts[i] != F32     # 4 x 8 blocks: 16-bit tensors with W % 8 == 0
            W = 8 * rng.randint(1, 5) if eight else 4 * rng.randint(1, 10)
            cases.append(dict(B=rng.randint(1, 5), C=chans[i], H=H, W=W, stride=1, pad=(1, 1, 1, 1), act=acts[i],
                              dtype=dts[i], want_mean=means[i], block_cols=cols[i] if cols[i] != 8 or eight else None))
        return cases

    def reference(self, c, inp):
        return self.module()._ref_and_bound(inp['x'], inp['w'], inp['b'], c['act'])

    def check(self, c, inp, got, mean=None):
        ref, bound = self.reference(c, inp)
        self.module()._check(ref, bound, got, mean, 'fuzz')

    def accept(self, lib, c, B=0, p=None):
        p = p or HOST
        cols = ctypes.c_int(0)
        return [lib.mtr_depthwise3x3_blocks_bias_act_opts(p.X, DT_CODE[c['dtype']], p.W, p.B, ACT_CODES[c['act']], B,
                                                          c['C'], c['H'], c['W'], p.Y, _opt(c['want_mean'], p.M), None,
                                                          c['block_cols'] or 0),
                lib.mtr_depthwise3x3_blocks_supported(DT_CODE[c['dtype']], c['H'], c['W'], 1, 1, 1, 1, 1,
                                                      ctypes.addressof(cols))]

    def supported(self, c, device='cpu', shift=0):
        from metrabs_amd import kernels
        return kernels.depthwise3x3_blocks_supported(c['dtype'], c['H'], c['W'], c['stride'], c['pad'], data_ptr=shift)

    def run(self, kernels, c, inp, out=None):
        return kernels.depthwise3x3_blocks_bias_act(inp['x'], inp['w'], inp['b'], c['act'], want_mean=c['want_mean'],
                                                    block_cols=c['block_cols'])


# ================================================================================================ K10 and the SE gate

class K10(Kernel):
    """bias_act_ (with and without a skip) and bias_act_rowmean_ (want_mean; it has no skip).  H * W is a multiple of
    the 16-byte vector (4 f32, 8 16-bit elements): the entry's rule."""
    name, seed = 'k10', 1001
    has_mean = True

    def module(self):
        import test_gpu_bias_act
        return test_gpu_bias_act

    def _generate(self, rng):
        chans, acts, dts = _channel_slots(rng, hi=600), _balanced(rng, ACTS), _balanced(rng, [F32, F16, BF16])
        means, ress = _balanced(rng, [False, True]), _balanced(rng, [False, True])
        cases = []
        for i in range(N_CASES):
            H, W = _draw_map(rng, 'any', group=4 if dts[i] == F32 else 8)
            cases.append(dict(B=rng.randint(1, 5), C=chans[i], H=H, W=W, act=acts[i], dtype=dts[i], want_mean=means[i],
                              residual=ress[i] and not means[i]))
        return cases

    def inputs(self, c, device, guard=False, seed=0):
        g = _gen(device, 6000 + seed)
        shape = (c['B'], c['C'], c['H'], c['W'])
        y = (torch.randn(shape, device=device, generator=g) * 3).to(c['dtype'])
        b = torch.randn(c['C'], device=device, generator=g)
        r = (torch.randn(shape, device=device, generator=g) * 2).to(c['dtype'])
        return _nan_guard(dict(x=y, b=b, r=r if c['residual'] else None), ('r',), guard)

    def reference(self, c, inp):
        return self.module()._ref_and_bound(inp['x'], inp['b'], inp['r'], c['act'])

    def check(self, c, inp, got, mean=None):
        self.module()._check(inp['x'], inp['b'], inp['r'], c['act'], got, mean, tag='fuzz')

    def wrong(self, c, inp):
        out = {}
        if c['C'] >= 2:
            b = inp['b'].clone()
            b[-1] = inp['b'][-2]
            out['bias_shift'] = self.reference(c, dict(inp, b=b))[0]
        self._residual_first(c, inp, out)
        return out

    def out_shape(self, c):
        return (c['B'], c['C'], c['H'], c['W'])

    def accept(self, lib, c, B=0, p=None):
        p = p or HOST
        if c['want_mean']:
            return [lib.mtr_bias_act_rowmean_nchw(p.Y, DT_CODE[c['dtype']], p.B, ACT_CODES[c['act']], B, c['C'],
                                                  c['H'] * c['W'], p.M, None)]
        return [lib.mtr_bias_act_nchw(p.Y, DT_CODE[c['dtype']], p.B, _opt(c['residual'], p.R), ACT_CODES[c['act']], B,
                                      c['C'], c['H'] * c['W'], None)]

    def run(self, kernels, c, inp, out=None):
        """In place on `out`, which holds a copy of the input."""
        if c['want_mean']:
            return kernels.bias_act_rowmean_(out, inp['b'], c['act'])
        return kernels.bias_act_(out, inp['b'], c['act'], residual=inp['r'])


class SeGate(Kernel):
    """C is a multiple of 4 (the entry's rule: 16-byte rows of the mean and of W1); S is free."""
    name, seed = 'se_gate', 1201
    PAIRS = [('silu', 'sigmoid'), ('relu', 'hardsigmoid'), ('silu', 'hardsigmoid'), ('relu', 'sigmoid')]

    def module(self):
        import test_gpu_se_gate2
        return test_gpu_se_gate2

    def _generate(self, rng):
        pairs, layouts = _balanced(rng, self.PAIRS), _balanced(rng, [False, True])
        configs = _balanced(rng, [-1, 0, 1, 2, 3])
        squeeze = [1] * 3 + [2 * rng.randint(1, 40) + 1 for _ in range(9)] + [rng.randint(2, 160) for _ in range(12)]
        rng.shuffle(squeeze)
        return [dict(B=rng.randint(1, 5), C=4 * rng.randint(1, 150), S=squeeze[i], act=pairs[i][0], gate_fn=pairs[i][1], dtype=F32,
                     w2t=layouts[i], config=configs[i]) for i in range(N_CASES)]

    def inputs(self, c, device, guard=False, seed=0):
        g = _gen(device, 7000 + seed)
        B, C, S = c['B'], c['C'], c['S']
        mean = torch.randn(B, C, device=device, generator=g)
        w1 = torch.randn(S, C, 1, 1, device=device, generator=g) / C ** 0.5
        b1 = 0.1 * torch.randn(S, device=device, generator=g)
        w2 = torch.randn(C, S, 1, 1, device=device, generator=g) / S ** 0.5
        b2 = 0.1 * torch.randn(C, device=device, generator=g)
        return _nan_guard(dict(x=mean, w=w1, b=b1, w2=w2, b2=b2), ('x',), guard)

    def _args(self, c, inp):
        return inp['x'], inp['w'], inp['b'], inp['w2'], inp['b2'], c['act'], c['gate_fn']

    def reference(self, c, inp):
        return self.module()._fp64_and_bound(*self._args(c, inp))

    def check(self, c, inp, got, mean=None):
        ref, bound = self.reference(c, inp)
        assert got.shape == ref.shape and got.dtype == F32
        excess = float(((got.double() - ref).abs() - bound).max())
        assert excess <= 0, excess

    def wrong(self, c, inp):
        out = {'last_channel': self.reference(c, dict(inp, x=inp['x'][:, :-1], w=inp['w'][:, :-1]))[0]}
        b2 = inp['b2'].clone()
        b2[-1] = inp['b2'][-2]
        out['bias_shift'] = self.reference(c, dict(inp, b2=b2))[0]
        return out

    def out_shape(self, c):
        return (c['B'], c['C'])

    def accept(self, lib, c, B=0, p=None):
        p = p or HOST
        code = {'sigmoid': 0, 'hardsigmoid': 1}[c['gate_fn']]
        return [lib.mtr_se_gate_opts(p.X, p.W, p.B, p.W1, p.B1, ACT_CODES[c['act']], code, B, c['C'], c['S'], p.Y, None,
                                     int(c['w2t']), c['config'])]

    def run(self, kernels, c, inp, out=None):
        w2t = inp['w2'].flatten(1).t().contiguous() if c['w2t'] else None
        return kernels.se_gate(inp['x'], inp['w'], inp['b'], inp['w2'], inp['b2'], c['act'], c['gate_fn'], out=out,
                               w2t=w2t, config=c['config'])


KERNELS = {k.name: k for k in (K13(), K13h(), K20(), K14h(), K19(), K22(), K16h(), K17(), K11(), K15(), K18(), K10(),
                               SeGate())}
MFMA = [n for n, k in KERNELS.items() if k.mfma]


# ---- just outside each domain: a smallest accepted case, and ONE rule broken at a time
#      name -> (the accepted case, [(what is broken, the changed fields, bytes x lies past a 16-byte boundary, bytes y
#      does, the entry's documented code)]); -2 MTR_E_SHAPE, -4 MTR_E_PARAM, -6 MTR_E_ALIGN

_GEMM_BASE = dict(B=1, K=8, M=8, H=4, W=4, act='relu', gate=False, residual=False, in_bias=False, in_act=None, dtype=F32)
_DENSE_BASE = dict(B=1, K=8, M=8, H=4, W=8, stride=1, act='relu', residual=False, dtype=F32)
_DW_BASE = dict(B=1, C=3, H=6, W=8, stride=1, pad=(1, 1, 1, 1), act='relu', dtype=F32, want_mean=False)
OUTSIDE = {
    'k13': (_GEMM_BASE, [('HW % 4', dict(H=3, W=6), 0, 0, -2), ('Cin % 4', dict(K=6), 0, 0, -2),
                         ('x 8 bytes past a 16-byte boundary', {}, 8, 0, -6), ('y 8 bytes past', {}, 0, 8, -6)]),
    'k13h': (dict(_GEMM_BASE, dtype=BF16), [('HW % 8', dict(H=3, W=4), 0, 0, -2), ('Cin % 8', dict(K=12), 0, 0, -2),
                                            ('x 8 bytes past a 16-byte boundary', {}, 8, 0, -6)]),
    'k20': (_GEMM_BASE, [('HW % 4', dict(H=3, W=6), 0, 0, -2), ('Cin % 4', dict(K=6), 0, 0, -2),
                         ('x 8 bytes past a 16-byte boundary', {}, 8, 0, -6)]),
    'k14h': (dict(_DENSE_BASE, dtype=F16), [('Cin % 8', dict(K=12), 0, 0, -2), ('W % 4', dict(W=6), 0, 0, -2),
                                            ('Wo % 4 at stride 2', dict(W=12, stride=2), 0, 0, -2),
                                            ('a stride of 3', dict(stride=3), 0, 0, -2),
                                            ('x 8 bytes past a 16-byte boundary', {}, 8, 0, -6)]),
    'k19': (_DENSE_BASE, [('H odd', dict(H=3), 0, 0, -2), ('W % 4', dict(W=6), 0, 0, -2), ('Cin % 4', dict(K=6), 0, 0, -2),
                          ('x 8 bytes past a 16-byte boundary', {}, 8, 0, -6)]),
    'k22': (dict(_DENSE_BASE, stride=2), [('H odd', dict(H=3), 0, 0, -2), ('(W / 2) % 4', dict(W=12), 0, 0, -2),
                                          ('Cin % 4', dict(K=6), 0, 0, -2),
                                          ('x 8 bytes past a 16-byte boundary', {}, 8, 0, -6)]),
    'k16h': (dict(_DENSE_BASE, Cmid=16, residual=None, dtype=F16, chain=True),
             [('Cin % 8', dict(K=12), 0, 0, -2), ('Cmid % 8', dict(Cmid=12), 0, 0, -2), ('Cout > 128', dict(M=136), 0, 0, -2),
              ('a stride of 3', dict(stride=3), 0, 0, -2), ('x 8 bytes past a 16-byte boundary', {}, 8, 0, -6)]),
    'k17': (dict(B=1, K=3, M=8, H=4, W=8, stride=2, act='relu', xdtype=F32, dtype=F32, preproc=False, interleaved=False),
            [('Cout % 8', dict(M=12), 0, 0, -2), ('W % 8', dict(W=12), 0, 0, -2), ('H odd', dict(H=3), 0, 0, -2),
             ('x 8 bytes past a 16-byte boundary', {}, 8, 0, -6)]),
    'k11': (_DW_BASE, [('OW % 4', dict(W=7), 0, 0, -2), ('a stride of 3', dict(stride=3), 0, 0, -4),
                       ('y 8 bytes past a 16-byte boundary', {}, 0, 8, -6)]),
    'k15': (dict(_DW_BASE, H=8, W=8, pad=(2, 2, 2, 2)),
            [('OW % 4', dict(W=7), 0, 0, -2), ('a stride of 3', dict(stride=3), 0, 0, -4),
             ('a padded plane of more than 112 rows', dict(H=120), 0, 0, -2),
             ('y 8 bytes past a 16-byte boundary', {}, 0, 8, -6)]),
    'k18': (dict(_DW_BASE, W=8, block_cols=None), [('W % 4', dict(W=6), 0, 0, -2),
                                                  ('x 8 bytes past a 16-byte boundary', {}, 8, 0, -6)]),
    'k10': (dict(B=1, C=3, H=2, W=4, act='relu', dtype=F32, want_mean=False, residual=False),
            [('HW % 4', dict(H=2, W=3), 0, 0, -2), ('y 8 bytes past a 16-byte boundary', {}, 0, 8, -6)]),
    'se_gate': (dict(B=1, C=8, S=2, act='relu', gate_fn='sigmoid', dtype=F32, w2t=False, config=-1),
                [('C % 4', dict(C=6), 0, 0, -2), ('the mean 8 bytes past a 16-byte boundary', {}, 8, 0, -6)]),
}


def case_id(c):
    return ' '.join(f'{k}={str(v).replace("torch.", "")}' for k, v in c.items())
